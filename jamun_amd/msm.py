"""Markov state model metrics of sampled trajectories: whether a sampler visits the metastable states of the true dynamics with the right
weights and hops between them at the right rates.

The last block of the reference's analysis pipeline (``analysis/utils.py``: ``compute_MSM_stats`` with
``compute_JSD_MSM_stats_against_time``, driven from ``analysis/run_analysis.py``): k-means on the TICA projection of the TRUE trajectory
(pyemma's ``cluster_kmeans(k=100, max_iter=100, fixed_seed=137)``), a Markov state model on the cluster labels (``estimate_markov_model``
at lag 1000), PCCA+ down to 10 metastable states, a coarse model on the metastable labels, and for the samples the metastable
occupancies, their Jensen-Shannon distance from the true ones (also against the number of samples) and a transition matrix at lag 10.
pyemma, msmtools and deeptime are not needed: the algorithms are written out below from their documentation.

    `assign_centers_host`, `cluster_sums_host`, `transition_counts_host`, `label_counts_host`
                                 the specification (numpy, float64 / int64) and the host path of the four reductions over frames
    ``native.assign_centers``, ``native.cluster_sums``, ``native.transition_counts``, ``native.label_counts`` (``jamun_msm.hip``)
                                 the device path: labels and counts integer for integer, distances and sums bit for bit the specification's
    `kmeans_init_host`, `kmeans` k-means++ on a subsample (host, both paths) and Lloyd's loop (either path, the same centres bit for bit)
    `estimate_msm`               largest connected set, reversible maximum-likelihood transition matrix, stationary vector, timescales
    `pcca`                       metastable sets of a reversible transition matrix (the inner simplex algorithm)
    `MSMMetrics`                 the meter `callbacks.MSMMetricsCallback` drives

WHERE THIS DEPARTS FROM PYEMMA (`DEPARTURES`, repeated in ``model.json``): the k-means++ draws come from ``np.random.RandomState(seed)``
on a strided subsample (pyemma's own stream of random numbers cannot be reproduced); PCCA stops at the inner simplex solution (msmtools
refines the transformation ``A`` by Nelder-Mead afterwards, which differs between scipy versions and is not needed for the crisp sets);
the reversible estimator is the plain fixed-point iteration to 1e-12.

Out of scope: plots, wandb, implied-timescale scans, Chapman-Kolmogorov tests, and gathering chains across ranks (each rank meters its own
walkers, as the other meters do).
"""

from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .meters import save_npz
from .native import MSM_MAX_D, MSM_MAX_K, MSM_MAX_KD, MSM_MAX_SEGMENTS, MSM_MAX_STATES, TICA_SLICE
from .tica import TICAMetrics, _as_numpy, js_distance_host

DEPARTURES = [
    "k-means++ initialisation draws from numpy.random.RandomState(seed) on a strided subsample of at most 65536 rows: pyemma's own random stream cannot be reproduced",
    "PCCA+ stops at the inner simplex solution (Weber and Galliat): msmtools' Nelder-Mead refinement of the transformation is left out (not deterministic across scipy versions, not needed for the crisp sets)",
    "the reversible maximum-likelihood estimate is the plain fixed-point iteration, stopped when the stationary vector moves by less than 1e-12",
    "metastable states are numbered by descending stationary weight",
]

ASSIGN_CHUNK = 1 << 14  # rows whose [rows, k] distances the host path holds at a time


# ---- the specification of the four reductions --------------------------------------------------------------------------------------------------

def assign_centers_host(y, centers) -> Tuple[np.ndarray, np.ndarray]:
    """``y [T, d]`` and ``centers [k, d]`` (finite) -> ``(labels int32 [T], sqdist float64 [T])``: the centre of smallest squared distance,
    the lowest index on a tie, and the distance to it.  The distance is accumulated column by column,
    ``acc += (y[:, j, None] - c[None, :, j]) * (y[:, j, None] - c[None, :, j])`` onto zeros: a subtraction, a multiplication and an
    addition, each rounded on its own.  A row with a non-finite value gets label -1 and distance NaN.  The specification of
    ``jamun_assign_centers``."""
    y = np.asarray(_as_numpy(y), dtype=np.float64)
    c = np.asarray(_as_numpy(centers), dtype=np.float64)
    if y.ndim != 2 or c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != y.shape[1]:
        raise ValueError(f"expected y [T, d] and centers [k, d] with k >= 1, got {y.shape} and {c.shape}")
    T, d = y.shape
    labels = np.empty(T, dtype=np.int32)
    sqdist = np.empty(T, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, T, ASSIGN_CHUNK):
            rows = y[t0 : t0 + ASSIGN_CHUNK]
            acc = np.zeros((rows.shape[0], c.shape[0]))
            for j in range(d):
                diff = rows[:, j, None] - c[None, :, j]
                acc += diff * diff
            finite = np.isfinite(rows).all(axis=1)
            acc[~finite] = 0.0
            best = np.argmin(acc, axis=1)
            labels[t0 : t0 + ASSIGN_CHUNK] = np.where(finite, best, -1)
            sqdist[t0 : t0 + ASSIGN_CHUNK] = np.where(finite, acc[np.arange(rows.shape[0]), best], np.nan)
    return labels, sqdist


def cluster_sums_host(y, labels, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """``y [T, d]`` (or ``[T]``: one column) and ``labels [T]`` -> ``(counts int64 [k], sums float64 [k, d])``: the rows carrying each label
    and their sum; labels outside ``[0, k)`` are skipped.  THE ORDER OF THE ADDITIONS is part of the specification: the frames are cut
    into slices of 1024; within a slice a cluster's rows are added in ascending frame order onto +0.0 (``np.add.at``); the slices are
    added in ascending order onto +0.0.  The specification of ``jamun_cluster_sums``."""
    y = np.asarray(_as_numpy(y), dtype=np.float64)
    if y.ndim == 1:
        y = y[:, None]
    labels = np.asarray(_as_numpy(labels)).reshape(-1)
    if y.ndim != 2 or labels.shape[0] != y.shape[0] or k < 1:
        raise ValueError(f"expected y [T, d], labels [T] and k >= 1, got {y.shape}, {labels.shape} and {k}")
    counts = np.zeros(k, dtype=np.int64)
    sums = np.zeros((k, y.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, y.shape[0], TICA_SLICE):
            lab = labels[t0 : t0 + TICA_SLICE]
            keep = (lab >= 0) & (lab < k)
            part = np.zeros_like(sums)
            np.add.at(part, lab[keep], y[t0 : t0 + TICA_SLICE][keep])
            sums += part
            counts += np.bincount(lab[keep], minlength=k).astype(np.int64)
    return counts, sums


def states_host(labels, n_states: int, state_map=None) -> np.ndarray:
    """The state of every label, -1 for none: the label itself if it lies in ``[0, n_states)``, or with ``state_map`` (``[n_in]``, -1 for
    none) ``state_map[label]`` for ``0 <= label < n_in`` if that lies in ``[0, n_states)``."""
    lab = np.asarray(_as_numpy(labels)).reshape(-1).astype(np.int64)
    if state_map is None:
        return np.where((lab >= 0) & (lab < n_states), lab, -1)
    m = np.asarray(_as_numpy(state_map)).reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < m.shape[0])
    s = np.where(ok, m[np.where(ok, lab, 0)], -1) if m.shape[0] else np.full_like(lab, -1)
    return np.where((s >= 0) & (s < n_states), s, -1)


def transition_counts_host(labels, lag: int, n_states: int, state_map=None, out: Optional[np.ndarray] = None) -> np.ndarray:
    """int64 ``[n_states, n_states]``: ``out[a, b]`` increased by the number of ``t < T - lag`` with ``state(t) = a`` and
    ``state(t + lag) = b`` (`states_host`; pairs with a -1 are skipped): pyemma's "sliding" counting.  ``out`` is added to (default zeros).
    The specification of ``jamun_transition_counts``."""
    if lag < 1:
        raise ValueError(f"lag must be at least 1, got {lag}")
    s = states_host(labels, n_states, state_map)
    out = np.zeros((n_states, n_states), dtype=np.int64) if out is None else out
    if lag < s.shape[0]:
        a, b = s[: s.shape[0] - lag], s[lag:]
        keep = (a >= 0) & (b >= 0)
        np.add.at(out, (a[keep], b[keep]), 1)
    return out


def label_counts_host(labels, bounds, n_states: int, state_map=None, out: Optional[np.ndarray] = None) -> np.ndarray:
    """int64 ``[n_seg, n_states]``: ``out[s, a]`` increased by the number of frames ``bounds[s] <= t < bounds[s + 1]`` in state ``a``
    (``bounds [n_seg + 1]`` non-decreasing within ``[0, T]``).  The specification of ``jamun_label_counts``."""
    s = states_host(labels, n_states, state_map)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1)
    if bounds.shape[0] < 2 or (np.diff(bounds) < 0).any() or bounds[0] < 0 or bounds[-1] > s.shape[0]:
        raise ValueError(f"bounds must be at least two non-decreasing integers within [0, {s.shape[0]}]")
    out = np.zeros((bounds.shape[0] - 1, n_states), dtype=np.int64) if out is None else out
    for i in range(bounds.shape[0] - 1):
        seg = s[bounds[i] : bounds[i + 1]]
        out[i] += np.bincount(seg[seg >= 0], minlength=n_states).astype(np.int64)
    return out


# ---- k-means --------------------------------------------------------------------------------------------------------------------------------------

def _on_gpu(y) -> bool:
    return torch.is_tensor(y) and y.is_cuda


def kmeans_init_host(y, k: int, seed: int = 137, max_rows: int = 65536) -> np.ndarray:
    """k-means++ on the rows ``y[::ceil(R / max_rows)]`` (only they are brought to the host where ``y`` is a device tensor) ->
    ``centers float64 [k_eff, d]``, ``k_eff <= k``.  ``rng = np.random.RandomState(seed)``; the first centre is row ``rng.randint(n)``;
    each next one is row ``searchsorted(cumsum(mindist), rng.rand() * total, side="right")`` (clipped to ``n - 1``, and walked back to
    the last row of positive distance should the clip land on a centre), ``mindist`` the squared distance of `assign_centers_host` to the
    nearest centre so far.  With ``total == 0`` (fewer distinct rows than ``k``) it stops with the centres found."""
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    R = int(y.shape[0])
    step = max(1, -(-R // int(max_rows)))
    x = np.ascontiguousarray(_as_numpy(y[::step]), dtype=np.float64)
    x = x[np.isfinite(x).all(axis=1)]
    n = x.shape[0]
    if n == 0:
        raise ValueError("no finite row to choose centres from")
    rng = np.random.RandomState(seed)
    chosen = [int(rng.randint(n))]
    mindist = assign_centers_host(x, x[chosen])[1]
    while len(chosen) < k:
        cum = np.cumsum(mindist)
        total = cum[-1]
        if not total > 0:
            break
        i = min(int(np.searchsorted(cum, rng.rand() * total, side="right")), n - 1)
        while mindist[i] == 0:
            i -= 1
        chosen.append(i)
        mindist = np.minimum(mindist, assign_centers_host(x, x[i : i + 1])[1])
    return np.ascontiguousarray(x[chosen])


def _assign(y, centers: np.ndarray, prev=None):
    """One assignment on the path of ``y``: ``(labels, sqdist, labels that differ from prev or None)``, labels and sqdist where ``y`` is."""
    if _on_gpu(y):
        from . import native

        labels, sq, n = native.assign_centers(y, centers, sqdist=True, prev_labels=prev)
        return labels, sq, None if n is None else int(n.item())
    labels, sq = assign_centers_host(y, centers)
    return labels, sq, None if prev is None else int(np.count_nonzero(labels != prev))


def _cluster_sums(y, labels, k: int) -> Tuple[np.ndarray, np.ndarray]:
    if _on_gpu(y):
        from . import native

        counts, sums = native.cluster_sums(y, labels, k)
        return counts.cpu().numpy(), sums.cpu().numpy()
    return cluster_sums_host(y, labels, k)


def kmeans(y, centers0, max_iter: int = 100) -> Dict[str, object]:
    """Lloyd's algorithm on the rows ``y [T, d]`` from the centres ``centers0 [k, d]``.  ``y`` is a float64 tensor on a GPU (the device
    path: ``y`` stays there; per iteration the number of changed labels, ``counts [k]`` and ``sums [k, d]`` come back) or an array / CPU
    tensor (the host path).  One iteration: assign every row to its nearest centre; count the labels that changed; stop if none did;
    else centre = sum / count of its rows (IEEE division on the host; an empty cluster keeps its centre).  At most ``max_iter``
    iterations.  Returns ``centers [k, d]``, ``n_iter``, ``converged``, ``inertia`` (the sum over clusters of the cluster sums of the
    squared distances to the final centres), ``labels`` (of the final centres, where ``y`` is) and ``counts [k]``.  Both reductions are
    bit-exact on either path, so THE TWO PATHS GIVE THE SAME CENTRES BIT FOR BIT on the same input."""
    centers = np.array(_as_numpy(centers0), dtype=np.float64, order="C")
    if centers.ndim != 2 or centers.shape[0] < 1 or y.ndim != 2 or centers.shape[1] != y.shape[1]:
        raise ValueError(f"expected y [T, d] and centers0 [k, d], got {tuple(y.shape)} and {centers.shape}")
    if not _on_gpu(y):
        y = np.asarray(_as_numpy(y), dtype=np.float64)
    k, T = centers.shape[0], int(y.shape[0])
    prev = torch.full((T,), -2, dtype=torch.int32, device=y.device) if _on_gpu(y) else np.full(T, -2, dtype=np.int32)
    n_iter, converged = 0, False
    while n_iter < max_iter:
        labels, _, changed = _assign(y, centers, prev)
        n_iter += 1
        prev = labels
        if changed == 0:
            converged = True
            break
        counts, sums = _cluster_sums(y, labels, k)
        filled = counts > 0
        centers[filled] = sums[filled] / counts[filled, None].astype(np.float64)
    labels, sqdist, _ = _assign(y, centers)
    counts, per_cluster = _cluster_sums(sqdist, labels, k)
    return {"centers": centers, "n_iter": n_iter, "converged": converged, "inertia": float(per_cluster[:, 0].sum()), "labels": labels, "counts": counts}


# ---- the Markov state model -------------------------------------------------------------------------------------------------------------------------

def largest_connected_set(counts: np.ndarray) -> np.ndarray:
    """The largest strongly connected set of the graph ``counts > 0`` as ascending state indices; of several of that size the one holding
    the lowest state."""
    n = counts.shape[0]
    reach = ((np.asarray(counts) > 0) | np.eye(n, dtype=bool)).astype(np.float32)
    while True:  # closure by repeated squaring: at most log2(n) rounds
        nxt = ((reach @ reach) > 0).astype(np.float32)
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    mutual = (reach > 0) & (reach.T > 0)
    best = np.zeros(0, dtype=np.int64)
    seen = np.zeros(n, dtype=bool)
    for i in range(n):
        if not seen[i]:
            members = np.flatnonzero(mutual[i])
            seen[members] = True
            if members.shape[0] > best.shape[0]:
                best = members
    return best


def estimate_msm(counts, reversible: bool = True, lag: Optional[int] = None, tol: float = 1e-12, max_iter: int = 100000) -> Dict[str, object]:
    """The Markov state model of a count matrix ``counts [n, n]``, restricted to its `largest_connected_set`: pyemma's default, the
    reversible maximum-likelihood estimate, by the fixed-point iteration

        x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j),    c_i = sum_j c_ij,  x_i = sum_j x_ij,   from x = C + C^T

    stopped when the largest change of ``x_i / sum x`` is below ``tol`` or after ``max_iter`` iterations; ``T_ij = x_ij / x_i``,
    ``pi_i = x_i / sum x``.  ``reversible=False`` gives ``C / rowsum`` with ``pi`` from the leading left eigenvector.  Returns
    ``active_set``, ``transition_matrix``, ``pi``, ``n_iter`` and ``timescales`` (``-lag / ln |lambda_i|`` for ``i >= 1``, eigenvalues by
    descending magnitude; None without ``lag``).  A ``ValueError`` where no state of the set has a counted transition ("no connected
    pair")."""
    C = np.asarray(counts, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1 or (C < 0).any() or not np.isfinite(C).all():
        raise ValueError(f"counts must be a square matrix of finite non-negative numbers, got {C.shape}")
    active = largest_connected_set(C)
    C = C[np.ix_(active, active)]
    c = C.sum(axis=1)
    if not (c > 0).all():
        raise ValueError("the count matrix has no connected pair of states: no transition was counted within a connected set")
    n_iter = 0
    if reversible:
        sym = C + C.T
        x = sym.copy()
        xi = x.sum(axis=1)
        pi = xi / xi.sum()
        while n_iter < max_iter:
            q = c / xi
            x = sym / (q[:, None] + q[None, :])
            xi = x.sum(axis=1)
            new = xi / xi.sum()
            n_iter += 1
            moved = float(np.abs(new - pi).max())
            pi = new
            if moved < tol:
                break
        T = x / xi[:, None]
        root = np.sqrt(pi)
        S = T * root[:, None] / root[None, :]
        lam = np.linalg.eigvalsh(0.5 * (S + S.T))
    else:
        T = C / c[:, None]
        w, v = np.linalg.eig(T.T)
        lead = np.real(v[:, int(np.argmax(np.real(w)))])
        pi = np.abs(lead) / np.abs(lead).sum()
        lam = np.linalg.eigvals(T)
    lam = lam[np.argsort(-np.abs(lam), kind="stable")]
    timescales = None
    if lag is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            timescales = -float(lag) / np.log(np.abs(lam[1:]))
    return {"active_set": active, "transition_matrix": T, "pi": pi, "n_iter": n_iter, "timescales": timescales}


def spread_model(model: Optional[dict], n: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(transition matrix [n, n], pi [n])`` of a model on an active set of ``range(n)``: the matrix spread into an identity, ``pi`` into
    zeros, as the reference does for a coarse model that misses states.  ``None`` gives the identity and zeros."""
    T, pi = np.eye(n), np.zeros(n)
    if model is not None:
        a = model["active_set"]
        T[np.ix_(a, a)] = model["transition_matrix"]
        pi[a] = model["pi"]
    return T, pi


def pcca_eigenvectors(T: np.ndarray, pi: np.ndarray, m: int) -> np.ndarray:
    """The leading ``m`` right eigenvectors ``[n, m]`` of the reversible ``T`` with stationary vector ``pi``, from the symmetric
    ``D^1/2 T D^-1/2`` (``D = diag(pi)``, ``eigh``): the first column is set to the constant 1, every other has unit ``pi``-norm and its
    entry of largest magnitude positive."""
    root = np.sqrt(pi)
    S = T * root[:, None] / root[None, :]
    lam, u = np.linalg.eigh(0.5 * (S + S.T))
    order = np.argsort(-lam, kind="stable")[:m]
    v = u[:, order] / root[:, None]
    big = np.argmax(np.abs(v), axis=0)
    v = v * np.where(v[big, np.arange(v.shape[1])] < 0, -1.0, 1.0)[None, :]
    v[:, 0] = 1.0
    return v


def pcca_memberships(v: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The inner simplex algorithm (Weber and Galliat 2002) on eigenvectors ``v [n, m]`` whose first column is constant:
    ``(memberships chi [n, m], vertices [m])``.  The first vertex is the row of largest norm with the constant column removed; each next
    one the row farthest from the affine span of those chosen (Gram-Schmidt); ``chi = v A`` with ``A`` the inverse of the vertex rows.
    Flipping the sign of a column of ``v`` flips a row of ``A``: ``chi`` does not depend on the signs.  ``ValueError`` where the rows
    span fewer than ``m - 1`` dimensions."""
    n, m = v.shape
    w = v[:, 1:]
    vertices = [int(np.argmax(np.sqrt((w * w).sum(axis=1))))]
    r = w - w[vertices[0]][None, :]
    scale = max(float(np.abs(w).max()), 1.0) if m > 1 else 1.0
    for _ in range(1, m):
        dist = np.sqrt((r * r).sum(axis=1))
        i = int(np.argmax(dist))
        if not dist[i] > 1e-10 * scale:
            raise ValueError("the eigenvector rows do not span a simplex of that many vertices")
        vertices.append(i)
        u = r[i] / dist[i]
        r = r - np.outer(r @ u, u)
    vertices = np.asarray(vertices, dtype=np.int64)
    return v @ np.linalg.inv(v[vertices]), vertices


def pcca(T, pi, m: int) -> Dict[str, object]:
    """The ``m`` metastable sets of the reversible transition matrix ``T [n, n]`` with stationary vector ``pi``: `pcca_eigenvectors`,
    `pcca_memberships`, the crisp assignment ``argmax chi`` (the lowest index on a tie).  The sets are numbered by descending stationary
    weight, ties by their lowest member.  With ``n < m`` states ``m`` is lowered to ``n``.  DEPARTURE FROM PYEMMA: msmtools follows this
    initial solution with a Nelder-Mead refinement of ``A``; it is left out (not deterministic across scipy versions, not needed for the
    crisp sets).  Returns ``m``, ``assignment int32 [n]``, ``memberships [n, m]``, ``weights [m]`` and ``vertices [m]``."""
    T, pi = np.asarray(T, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    n = T.shape[0]
    if T.shape != (n, n) or pi.shape != (n,) or m < 1 or not (pi > 0).all():
        raise ValueError(f"expected T [n, n], a positive pi [n] and m >= 1, got {T.shape}, {pi.shape} and {m}")
    m = min(int(m), n)
    chi, vertices = pcca_memberships(pcca_eigenvectors(T, pi, m))
    crisp = np.argmax(chi, axis=1)
    weight = np.array([pi[crisp == s].sum() for s in range(m)])
    first = np.array([np.flatnonzero(crisp == s)[0] if (crisp == s).any() else n for s in range(m)])
    order = np.lexsort((first, -weight))  # (the last key sorts first)
    rank = np.empty(m, dtype=np.int64)
    rank[order] = np.arange(m)
    return {"m": m, "assignment": rank[crisp].astype(np.int32), "memberships": chi[:, order], "weights": weight[order], "vertices": vertices[order]}


def sample_steps(T: int, n_steps: int) -> np.ndarray:
    """The reference's prefixes of ``T`` frames: the unique values of ``np.logspace(0, log10(T), n_steps, dtype=int)``."""
    return np.unique(np.logspace(0, np.log10(T), n_steps, dtype=int)).astype(np.int64)


def _probs(counts: np.ndarray) -> np.ndarray:
    total = counts.sum()
    return counts / total if total > 0 else np.full(counts.shape, np.nan)


# ---- the meter ------------------------------------------------------------------------------------------------------------------------------------------

class MSMMetrics(TICAMetrics):
    """The meter of one dataset: TICA, k-means, a Markov state model and its metastable states fitted on the reference trajectory, and per
    chain and for the joined trajectory the occupancies of the metastable states, their Jensen-Shannon distance from the reference's
    (for the whole trajectory and for ``n_steps`` log-spaced prefixes) and the transition counts and matrix at ``traj_lag``, written
    under ``<output_dir>/<label>/msm/`` on rank 0:

        model.json      the options, k_eff, the k-means iterations and whether it converged, the sizes of the active sets, the estimator's
                        iterations, `DEPARTURES`, and ``note``: why no model was fitted, or what was lowered, or null
        model.npz       centers [k_eff, d], metastable_map [k_eff] (microstate -> metastable state, -1 outside the active set),
                        msm_transition_matrix [n_metastable, n_metastable] and msm_pi [n_metastable] (the coarse model, spread into an
                        identity / zeros), timescales (of the microstate model), inertia
        true_traj.npz   metastable_probs [n_metastable], num_frames, unassigned_frames, steps, js_vs_samples
        <i>.npz         per chain: metastable_probs, js_distance_metastable_probs, transition_counts, traj_transition_matrix, traj_pi,
                        steps, js_vs_samples, num_frames, nonfinite_frames, unassigned_frames
        joined.npz      the same for all chains so far in running order

    The TICA model is `TICAMetrics`' (its options ``lag``, ``features``, ``var_cutoff``, ``epsilon``, ``kinetic_map``, ``reference``); the
    whole projection of the reference stays on the compute device; k-means (`kmeans_init_host`, `kmeans`), the microstate model at
    ``msm_lag`` (`estimate_msm`), `pcca` to ``n_metastable`` states and the coarse model on the metastable labels follow.  Without a
    reference, with one no longer than a lag, with a non-finite reference feature or a count matrix with no connected pair no model is
    fitted: ``model.json`` carries the reason in ``note``, nothing else is written and `compute` returns ``{}``.

    Of a chain only the ``[n_metastable, n_metastable]`` transition counts, the occupancy counts of the segments between the steps and
    the count of non-finite rows come to the host.  A frame labelled -1 (a non-finite row, or a microstate outside the active set) is in
    no occupancy and in no pair, and counted in ``unassigned_frames``.  THE JOINED TRANSITION COUNTS are the sum of the chains' counts,
    never the counts of the concatenated frames: no pair crosses from one chain into the next.  ``traj_transition_matrix`` / ``traj_pi``
    are the reversible estimate on the counts, spread as above (the identity and zeros where the counts connect no pair).

    ``device`` as in `TICAMetrics`; the device path needs its conditions and ``k <= 1024``, ``k d <= 16384``, ``n_metastable <= 1024``,
    ``n_steps <= 4094``.  `compute` returns ``{"<label>/msm/js_distance_metastable_probs_joined": the joined trajectory's value}``."""

    DIRECTORY = "msm"

    def __init__(self, dataset, k: int = 100, max_iter: int = 100, seed: int = 137, msm_lag: int = 1000, n_metastable: int = 10,
                 traj_lag: int = 10, n_steps: int = 50, lag: int = 1000, features: str = "all", var_cutoff: float = 0.95, epsilon: float = 1e-6,
                 kinetic_map: bool = True, reference=None, device: str = "auto", output_dir: str = "sampler", sample_key: str = "xhat_traj", **_):
        super().__init__(dataset, lag=lag, max_acf_lag=0, features=features, var_cutoff=var_cutoff, epsilon=epsilon, kinetic_map=kinetic_map,
                         reference=reference, device=device, output_dir=output_dir, sample_key=sample_key)
        for name, value, low in (("k", k, 1), ("max_iter", max_iter, 1), ("seed", seed, 0), ("msm_lag", msm_lag, 1), ("n_metastable", n_metastable, 1),
                                 ("traj_lag", traj_lag, 1), ("n_steps", n_steps, 1)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low:
                raise ValueError(f"{name} must be an integer of at least {low}, got {value!r}")
        self.k, self.max_iter, self.seed, self.msm_lag = int(k), int(max_iter), int(seed), int(msm_lag)
        self.n_metastable, self.traj_lag, self.n_steps = int(n_metastable), int(traj_lag), int(n_steps)
        self.msm: Optional[dict] = None  # centers, map, true_probs, ...
        self._records: List[dict] = []   # per chain: labels (where they were computed), counts, frames, nonfinite

    def _device_fits(self) -> bool:
        d = 1 if self.model is None else int(self.model["d"])
        return (super()._device_fits() and self.k <= MSM_MAX_K and d <= MSM_MAX_D and self.k * d <= MSM_MAX_KD and self.n_metastable <= MSM_MAX_STATES
                and self.n_steps + 2 <= MSM_MAX_SEGMENTS)

    def _device_needs(self) -> str:
        return (f"MSMMetrics(device='device') needs float32 sample tensors on a GPU, 1 to 128 feature columns (these are {self.width}), "
                f"k <= {MSM_MAX_K}, k * d <= {MSM_MAX_KD}, n_metastable <= {MSM_MAX_STATES} and n_steps <= {MSM_MAX_SEGMENTS - 2}")

    # ---- the two paths -----------------------------------------------------------------------------------------------------------------------------

    def _msm_tables(self, dev):
        """(centres, microstate -> metastable map) on ``dev``, uploaded once."""
        key = ("msm", str(dev))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.msm["centers"]).to(dev), torch.from_numpy(self.msm["map"]).to(dev))
        return self._dev[key]

    def _labels_of(self, proj):
        """Microstate labels of a projection, where it is."""
        if _on_gpu(proj):
            from . import native

            return native.assign_centers(proj, self._msm_tables(proj.device)[0])[0]
        return assign_centers_host(proj, self.msm["centers"])[0]

    def _map_on(self, labels, state_map: Optional[np.ndarray]):
        """The state map where the labels are (the model's own map is uploaded once)."""
        return self._msm_tables(labels.device)[1] if state_map is not None and _on_gpu(labels) else state_map

    def _transitions(self, labels, lag: int, n_states: int, state_map: Optional[np.ndarray]) -> np.ndarray:
        if _on_gpu(labels):
            from . import native

            return native.transition_counts(labels, lag, n_states, state_map=self._map_on(labels, state_map)).cpu().numpy()
        return transition_counts_host(labels, lag, n_states, state_map)

    def _occupancy(self, labels, bounds: np.ndarray, out=None):
        """Segment counts of the metastable states, added to ``out`` where the labels are."""
        n = self.n_metastable
        if _on_gpu(labels):
            from . import native

            return native.label_counts(labels, bounds.astype(np.int32), n, state_map=self._map_on(labels, self.msm["map"]), out=out)
        return label_counts_host(labels, bounds, n, self.msm["map"], out)

    @staticmethod
    def _bounds(T: int, steps: np.ndarray) -> np.ndarray:
        """Segment bounds whose prefixes are ``steps``, and whose last is ``T``."""
        b = np.concatenate([[0], steps])
        return np.concatenate([b, [T]]) if b[-1] < T else b

    def _against_steps(self, chains: List[Tuple[object, int]], true_probs: Optional[np.ndarray]) -> dict:
        """``chains``: (labels, frames) in running order -> steps, the occupancy counts of the whole and ``js_vs_samples`` over the prefixes."""
        total = sum(T for _, T in chains)
        steps = sample_steps(total, self.n_steps)
        bounds = self._bounds(total, steps)
        out, off = None, 0
        for labels, T in chains:
            out = self._occupancy(labels, np.clip(bounds - off, 0, T), out)
            off += T
        seg = self._host(out).astype(np.int64)
        prefix = np.cumsum(seg, axis=0)[: steps.shape[0]]
        occupancy = seg.sum(axis=0)
        ref = _probs(occupancy) if true_probs is None else true_probs
        return {"steps": steps, "occupancy": occupancy, "js_vs_samples": np.array([js_distance_host(p, ref) for p in prefix])}

    # ---- protocol ------------------------------------------------------------------------------------------------------------------------------------

    def _fit_msm(self, ref) -> Optional[str]:
        """Everything behind the TICA model; returns the reason where no model can be fitted."""
        R = int(ref.shape[0])
        if R <= self.msm_lag:
            return f"the reference has {R} frames, the lag of the Markov state model is {self.msm_lag}: no pair of frames to count"
        chunks = [self._project(self._features(self._on_compute_device(ref[t0 : t0 + self.REFERENCE_CHUNK])))[0] for t0 in range(0, R, self.REFERENCE_CHUNK)]
        y = chunks[0] if len(chunks) == 1 else (torch.cat(chunks) if torch.is_tensor(chunks[0]) else np.concatenate(chunks))
        km = kmeans(y, kmeans_init_host(y, self.k, self.seed), self.max_iter)
        k_eff = km["centers"].shape[0]
        labels = km["labels"]
        try:
            micro = estimate_msm(self._transitions(labels, self.msm_lag, k_eff, None), lag=self.msm_lag)
        except ValueError as e:
            return f"no microstate model: {e}"
        try:
            sets = pcca(micro["transition_matrix"], micro["pi"], self.n_metastable)
        except ValueError as e:
            return f"no metastable states: {e}"
        state_map = np.full(k_eff, -1, dtype=np.int32)
        state_map[micro["active_set"]] = sets["assignment"]
        self.msm = {"centers": km["centers"], "map": state_map}
        notes = []
        if k_eff < self.k:
            notes.append(f"the reference has fewer distinct rows than k = {self.k}: k_eff = {k_eff}")
        if sets["m"] < self.n_metastable:
            notes.append(f"{micro['active_set'].shape[0]} active microstates: {sets['m']} metastable states instead of {self.n_metastable}")
        try:
            coarse = estimate_msm(self._transitions(labels, self.msm_lag, self.n_metastable, state_map), lag=self.msm_lag)
        except ValueError as e:
            self.msm = None
            return f"no coarse model: {e}"
        true = self._against_steps([(labels, R)], None)
        T, pi = spread_model(coarse, self.n_metastable)
        self.msm.update(k_eff=k_eff, kmeans_iterations=km["n_iter"], kmeans_converged=km["converged"], inertia=km["inertia"],
                        micro_active=int(micro["active_set"].shape[0]), coarse_active=int(coarse["active_set"].shape[0]), n_metastable_found=sets["m"],
                        micro_iterations=micro["n_iter"], coarse_iterations=coarse["n_iter"], timescales=micro["timescales"],
                        transition_matrix=T, pi=pi, true_probs=_probs(true["occupancy"]), true_steps=true["steps"], true_js=true["js_vs_samples"],
                        true_frames=R, true_unassigned=R - int(true["occupancy"].sum()))
        return "; ".join(notes) if notes else None

    def on_sample_start(self):
        ref = self._reference_frames(self.n_atoms, "the reference frames of", self.reference)
        self.note = self._fit(ref)
        if self.model is not None:
            self.note = self._fit_msm(ref)
        if not self._is_rank_zero():
            return
        d = self._dir()
        m = self.msm
        with open(os.path.join(d, "model.json"), "w") as f:
            json.dump({"k": self.k, "max_iter": self.max_iter, "seed": self.seed, "msm_lag": self.msm_lag, "n_metastable": self.n_metastable,
                       "traj_lag": self.traj_lag, "n_steps": self.n_steps, "lag": self.lag, "features": self.features, "var_cutoff": self.var_cutoff,
                       "epsilon": self.epsilon, "kinetic_map": self.kinetic_map, "feature_labels": self.feature_labels,
                       "d": None if self.model is None else int(self.model["d"]),
                       "k_eff": None if m is None else int(m["k_eff"]), "kmeans_iterations": None if m is None else int(m["kmeans_iterations"]),
                       "kmeans_converged": None if m is None else bool(m["kmeans_converged"]),
                       "active_microstates": None if m is None else m["micro_active"], "active_metastable_states": None if m is None else m["coarse_active"],
                       "metastable_states_found": None if m is None else int(m["n_metastable_found"]),
                       "estimator": "reversible", "estimator_iterations": None if m is None else [int(m["micro_iterations"]), int(m["coarse_iterations"])],
                       "departures_from_pyemma": DEPARTURES, "note": self.note}, f, indent=1)
        if m is not None:
            save_npz(os.path.join(d, "model.npz"), centers=m["centers"], metastable_map=m["map"], msm_transition_matrix=m["transition_matrix"],
                     msm_pi=m["pi"], timescales=m["timescales"], inertia=np.asarray(m["inertia"]))
            save_npz(os.path.join(d, "true_traj.npz"), metastable_probs=m["true_probs"], num_frames=np.asarray(m["true_frames"], dtype=np.int64),
                     unassigned_frames=np.asarray(m["true_unassigned"], dtype=np.int64), steps=m["true_steps"], js_vs_samples=m["true_js"])

    def update(self, sample) -> None:
        index, frames, off = self._next_chain(sample)
        T = int(frames.shape[0])
        if T == 0 or self.msm is None:
            return
        proj, nonfinite = self._project(self._features(frames))
        labels = self._labels_of(proj)
        self.joined_frames = off + T
        self._pending.append({"index": index, "frames": T, "nonfinite": nonfinite, "labels": labels,
                              "counts": self._transitions(labels, self.traj_lag, self.n_metastable, self.msm["map"])})

    def _arrays(self, chains: List[dict]) -> dict:
        steps = self._against_steps([(c["labels"], c["frames"]) for c in chains], self.msm["true_probs"])
        counts = np.sum([c["counts"] for c in chains], axis=0)
        try:
            model = estimate_msm(counts, lag=self.traj_lag)
        except ValueError:
            model = None
        T, pi = spread_model(model, self.n_metastable)
        frames = sum(c["frames"] for c in chains)
        return {"metastable_probs": _probs(steps["occupancy"]),
                "js_distance_metastable_probs": np.asarray(js_distance_host(steps["occupancy"], self.msm["true_probs"])), "transition_counts": counts,
                "traj_transition_matrix": T, "traj_pi": pi, "steps": steps["steps"], "js_vs_samples": steps["js_vs_samples"],
                "num_frames": np.asarray(frames, dtype=np.int64), "nonfinite_frames": np.asarray(sum(c["nonfinite"] for c in chains), dtype=np.int64),
                "unassigned_frames": np.asarray(frames - int(steps["occupancy"].sum()), dtype=np.int64)}

    def compute(self) -> Dict[str, float]:
        """Writes ``<i>.npz`` of the chains seen since the last call and ``joined.npz`` (rank 0) and returns the joined trajectory's
        Jensen-Shannon distance of the metastable occupancies."""
        pending, write, d = self._take_pending()
        if self.msm is None:
            return {}
        for rec in pending:
            self._records.append(rec)
            if write:
                save_npz(os.path.join(d, f"{rec['index']}.npz"), **self._arrays([rec]))
        if pending:
            joined = self._arrays(self._records)
            self._last_joined = float(joined["js_distance_metastable_probs"])
            if write:
                save_npz(os.path.join(d, "joined.npz"), **joined)
        return {} if self._last_joined is None else {f"{self.label}/msm/js_distance_metastable_probs_joined": self._last_joined}
