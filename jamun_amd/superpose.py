"""Rigid superposition of trajectory frames on a reference structure, and the per-frame RMSD to it.

The sampler removes translation (it mean-centres) but each walker's orientation diffuses freely, so a trajectory as sampled is a
tumbling molecule.  Every consumer of the reference's trajectories superposes first (mdtraj's ``Trajectory.superpose`` against the
dataset's first frame, ``metrics/_visualize_samples.py:26-28``, ``metrics/_trajectory_animation.py:70``).
That is, per frame: the PROPER rotation R (det +1, never a reflection) and the translation that minimise
``sum_i |R (x_i - c_x) + c_ref - ref_i|^2``, with c the centroids, and ``rmsd = sqrt(mean_i |aligned_i - ref_i|^2)``.

`superpose_host` is the specification (numpy, float64, Kabsch by SVD with the determinant correction) and the host path;
``native.superpose_frames`` (``jamun_superpose.hip``: Horn's quaternion matrix, Jacobi eigenvector, one lane per frame) is the device
path.  `superpose` picks between them.  Where the covariance is rank deficient (one or two atoms, collinear atoms) the rotation about
the free axis is arbitrary: the two paths then agree on the RMSD and on the shape of the aligned frame, not on its coordinates.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import torch


def _as_numpy(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def superpose_host(frames, ref) -> Tuple[np.ndarray, np.ndarray]:
    """``frames [T, n, 3]`` aligned on ``ref [n, 3]`` (any float type, tensors or arrays; nm): ``(aligned float32 [T, n, 3], rmsd float32 [T])``.
    A frame with a non-finite value comes back all NaN with a NaN rmsd; the other frames do not notice."""
    x = np.asarray(_as_numpy(frames), dtype=np.float64)
    r = np.asarray(_as_numpy(ref), dtype=np.float64)
    if x.ndim != 3 or x.shape[2] != 3 or r.shape != (x.shape[1], 3):
        raise ValueError(f"expected frames [T, n, 3] and ref [n, 3], got {x.shape} and {r.shape}")
    T, n = x.shape[0], x.shape[1]
    aligned = np.full((T, n, 3), np.nan)
    rmsd = np.full((T,), np.nan)
    if n == 0:
        return aligned.astype(np.float32), np.zeros((T,), dtype=np.float32)
    ok = np.isfinite(x).all(axis=(1, 2))
    if ok.any() and np.isfinite(r).all():
        xs = x[ok]
        c_ref = r.mean(axis=0)
        rc = r - c_ref
        xc = xs - xs.mean(axis=1, keepdims=True)
        h = np.einsum("tia,ib->tab", xc, rc)  # covariance of the centred coordinates: rows of xc @ rot approach rc
        u, _, vt = np.linalg.svd(h)
        d = np.sign(np.linalg.det(u) * np.linalg.det(vt))
        d[d == 0] = 1.0
        u[:, :, 2] *= d[:, None]  # the determinant correction: the best PROPER rotation (flip the direction of least covariance)
        rot = u @ vt
        out = xc @ rot + c_ref
        aligned[ok] = out
        rmsd[ok] = np.sqrt(((out - r) ** 2).sum(axis=(1, 2)) / n)
    return aligned.astype(np.float32), rmsd.astype(np.float32)


def superpose(frames, ref):
    """The public call: ``(aligned [T, n, 3], rmsd [T])`` of ``frames [T, n, 3]`` on ``ref [n, 3]``.  Float32 tensors on a GPU are aligned
    there by the HIP kernel (no copy of a strided chain view) when the native library loads; everything else goes through
    `superpose_host`.  Tensors in, tensors out (on the device of ``frames``); arrays in, arrays out."""
    if torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.float32:
        from . import _lib, native

        if _lib.available():
            ref_d = torch.as_tensor(ref, dtype=torch.float32, device=frames.device) if not torch.is_tensor(ref) else ref.to(frames.device, torch.float32)
            return native.superpose_frames(frames, ref_d)
    aligned, rmsd = superpose_host(frames, ref)
    if torch.is_tensor(frames):
        return torch.from_numpy(aligned).to(frames.device), torch.from_numpy(rmsd).to(frames.device)
    return aligned, rmsd
