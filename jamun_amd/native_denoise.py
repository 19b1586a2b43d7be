"""The two ends of a denoising evaluation around the forward: the binding of ``csrc/jamun_denoise.cpp`` (``jamun_denoise.hip``) and its
host mirrors.

`noise_align_graphs` noises a ragged batch of clean frames, centres them and aligns the noisy frames on the clean ones
(``Denoiser.noise_and_denoise``, ``src/jamun/model/denoiser.py:228-244``; ``utils/align.py:9-56``); `denoise_loss` reduces denoised frames to
the per-graph raw loss, scaled RMSD and weighted loss (``Denoiser.compute_loss``, ``denoiser.py:262-281``).  Tensors on a GPU go through the
HIP library; tensors on the CPU go through `noise_align_graphs_host` / `denoise_loss_host` (numpy), which are also what the tests hold the
kernels to: the noise and centring steps in the kernel's own fp32 operations, in its order (bit for bit), the alignment in float64 by SVD
with the determinant fix (the kernel: Horn's quaternion in fp32, within 1e-5 nm), the sums of the losses sequentially in fp32.

Every argument is checked before any GPU call and each refusal is a ``RuntimeError`` that names the argument.  ``ptr`` is read on the host
(it has to ascend from 0 to N): a table kept on the CPU, as `WalkerBatch` keeps it, costs nothing; one on the GPU is copied back first.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .native_frames import _call, _fit_31_bits, _ptr, _result

_F = np.float32


# ---- checks --------------------------------------------------------------------------------------------------------------------------

def _coords(name: str, t, device=None, n: Optional[int] = None) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise RuntimeError(f"{name} must be a tensor, got {type(t).__name__}")
    if device is not None and t.device != device:
        raise RuntimeError(f"{name} must be on {device} like x, got {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    if t.ndim != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise RuntimeError(f"{name} must be [{'N' if n is None else n}, 3], got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous, got strides {tuple(t.stride())}")
    return t


def _check_ptr(ptr, n_atoms: int) -> np.ndarray:
    """``ptr [W + 1]`` as an int32 host array: integers ascending (not strictly: a graph may be empty) from 0 to ``n_atoms``."""
    if torch.is_tensor(ptr):
        if ptr.is_floating_point() or ptr.dtype == torch.bool:
            raise RuntimeError(f"ptr must hold integers, got {ptr.dtype}")
        p = ptr.detach().cpu().numpy()
    else:
        p = np.asarray(ptr)
        if p.dtype.kind not in "iu":
            raise RuntimeError(f"ptr must hold integers, got {p.dtype}")
    if p.ndim != 1 or p.size < 1:
        raise RuntimeError(f"ptr must be [W + 1] with W >= 0, got {tuple(p.shape)}")
    p = p.astype(np.int64)
    if p[0] != 0 or p[-1] != n_atoms:
        raise RuntimeError(f"ptr must run from 0 to N = {n_atoms}, got ptr[0] = {int(p[0])}, ptr[-1] = {int(p[-1])}")
    if (np.diff(p) < 0).any():
        raise RuntimeError(f"ptr must be monotone, got a descent at graph {int(np.argmax(np.diff(p) < 0))}")
    _fit_31_bits(f"{p.size - 1} graphs of {n_atoms} atoms: the number of graphs and 3 N must fit 31 bits", p.size, 3 * n_atoms + 65536)
    return p.astype(np.int32)


def _check_sigma(sigma) -> float:
    s = float(sigma)
    if not math.isfinite(s) or not s > 0.0:
        raise RuntimeError(f"sigma must be finite and above 0, got {s}")
    return s


def _device_ptr(ptr, host: np.ndarray, device) -> torch.Tensor:
    if torch.is_tensor(ptr) and ptr.device == device and ptr.dtype == torch.int32 and ptr.is_contiguous():
        return ptr
    return torch.from_numpy(host).to(device)


# ---- host mirrors (numpy, no GPU) ----------------------------------------------------------------------------------------------------

def _as_f32(a) -> np.ndarray:
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)


def _centroid_f32(a: np.ndarray) -> np.ndarray:
    """k_mean_center's centroid of ``a [n, 3]``: the sequential fp32 sum in atom order, divided by n."""
    return np.add.accumulate(a, axis=0, dtype=np.float32)[-1] / _F(a.shape[0])


def kabsch_f64(y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """``utils/align.py:30-55`` for one graph in float64: ``R y + t`` with the proper rotation and the translation that bring ``y [n, 3]``
    closest to ``x [n, 3]``; the determinant fix flips the direction of the smallest singular value."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    y_mu, x_mu = y.mean(axis=0), x.mean(axis=0)
    H = (y - y_mu).T @ (x - x_mu)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return (y - y_mu) @ R.T + x_mu


def noise_align_graphs_host(x, noise, ptr, sigma, mean_center: bool = True, align: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(x_c, y, rmsd)`` float32 of `noise_align_graphs` on the host: the noise and centring steps in k_noise_align's fp32 operations and
    order (x_c, and y without ``align``, are the kernel's bits), the alignment in float64 (`kabsch_f64`), the RMSD of the float32 ``y``
    to ``x_c`` in float64.  A graph without atoms has rmsd 0."""
    x, noise = _as_f32(x), _as_f32(noise)
    p = _check_ptr(ptr, x.shape[0])
    s = _F(_check_sigma(sigma))
    x_c, y = np.empty_like(x), np.empty_like(x)
    rmsd = np.zeros(p.size - 1, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(p.size - 1):
            lo, hi = int(p[g]), int(p[g + 1])
            if hi == lo:
                continue
            xg = x[lo:hi]
            xc = xg - _centroid_f32(xg) if mean_center else xg.copy()
            yg = xc + s * noise[lo:hi]
            if mean_center:
                yg = yg - _centroid_f32(yg)
            if align:
                yg = kabsch_f64(yg, xc).astype(np.float32) if np.isfinite(yg).all() and np.isfinite(xc).all() else np.full_like(yg, np.nan)
            x_c[lo:hi], y[lo:hi] = xc, yg
            d = yg.astype(np.float64) - xc.astype(np.float64)
            rmsd[g] = np.sqrt((d * d).sum() / (hi - lo))
    return x_c, y, rmsd


def denoise_loss_host(xhat, x, ptr, sigma, inv_c_out_sq, loss_weight=None) -> np.ndarray:
    """``[W, 3]`` float32 (raw_coordinate_loss, scaled_rmsd, coordinate_loss) of `denoise_loss` on the host, in k_denoise_loss's fp32
    operations: the per-atom terms added in atom order."""
    xhat, x = _as_f32(xhat), _as_f32(x)
    p = _check_ptr(ptr, x.shape[0])
    scale = _F(_check_sigma(sigma)) * _F(1.7320508075688772)
    W = p.size - 1
    lw = np.ones(W, dtype=np.float32) if loss_weight is None else _as_f32(loss_weight).reshape(W)
    d = xhat - x
    r = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid="ignore"):
        t = np.sqrt(r) / scale
    out = np.zeros((W, 3), dtype=np.float32)
    for g in range(W):
        lo, hi = int(p[g]), int(p[g + 1])
        if hi == lo:
            continue
        out[g, 0] = np.add.accumulate(r[lo:hi], dtype=np.float32)[-1] / _F(hi - lo)
        out[g, 1] = np.add.accumulate(t[lo:hi], dtype=np.float32)[-1] / _F(hi - lo)
    out[:, 2] = (out[:, 0] * lw) * _F(inv_c_out_sq)
    return out


# ---- the binding ----------------------------------------------------------------------------------------------------------------------

def mean_center_graphs(x: torch.Tensor, ptr) -> torch.Tensor:
    """``x - centroid(graph)`` where ``x`` lives: `native.mean_center` (k_mean_center) on a GPU, the same fp32 operations in numpy on the
    CPU.  The x_c of `noise_align_graphs`, bit for bit."""
    x = _coords("x", x)
    p = _check_ptr(ptr, int(x.shape[0]))
    if x.is_cuda:
        from . import native

        return native.mean_center(x, _device_ptr(ptr, p, x.device))
    h, out = _as_f32(x), np.empty((x.shape[0], 3), dtype=np.float32)
    for g in range(p.size - 1):
        if p[g + 1] > p[g]:
            out[p[g] : p[g + 1]] = h[p[g] : p[g + 1]] - _centroid_f32(h[p[g] : p[g + 1]])
    return torch.from_numpy(out)


def noise_align_graphs(x: torch.Tensor, noise: torch.Tensor, ptr, sigma: float, mean_center: bool = True, align: bool = True,
                       out_x: Optional[torch.Tensor] = None, out_y: Optional[torch.Tensor] = None, rmsd: Optional[torch.Tensor] = None):
    """Queue ``x_c = x - centroid(x)``, ``y = x_c + sigma noise``, ``y -= centroid(y)`` (both centrings only with ``mean_center``) and the
    rigid alignment of ``y`` on ``x_c`` (only with ``align``) for the graphs ``ptr [W + 1]`` of ``x, noise [N, 3]`` (float32) on the
    current stream; returns ``(x_c [N, 3], y [N, 3], rmsd [W])``, the RMSD of ``y`` to ``x_c`` after the step (0 for a graph without
    atoms).  ``out_x`` / ``out_y`` / ``rmsd`` receive the results (default: new tensors).  Tensors on the CPU take the host mirror.
    See ``jamun_noise_align_graphs``."""
    x = _coords("x", x)
    N, dev = int(x.shape[0]), x.device
    noise = _coords("noise", noise, dev, N)
    p = _check_ptr(ptr, N)
    s = _check_sigma(sigma)
    W = p.size - 1
    out_x = _result("out_x", out_x, (N, 3), torch.float32, dev)
    out_y = _result("out_y", out_y, (N, 3), torch.float32, dev)
    rmsd = _result("rmsd", rmsd, (W,), torch.float32, dev)
    if not x.is_cuda:
        hx, hy, hr = noise_align_graphs_host(x, noise, p, s, mean_center, align)
        out_x.copy_(torch.from_numpy(hx)), out_y.copy_(torch.from_numpy(hy)), rmsd.copy_(torch.from_numpy(hr))
        return out_x, out_y, rmsd
    if W == 0 or N == 0:
        rmsd.zero_()
        return out_x, out_y, rmsd
    if (np.diff(p) == 0).any():
        rmsd.zero_()  # (a graph without atoms: the call writes nothing)
    _call(dev, "jamun_noise_align_graphs", _ptr(x), _ptr(noise), _ptr(_device_ptr(ptr, p, dev)), W, N, C.c_float(s), int(bool(mean_center)),
          int(bool(align)), _ptr(out_x), _ptr(out_y), _ptr(rmsd))
    return out_x, out_y, rmsd


def denoise_loss(xhat: torch.Tensor, x: torch.Tensor, ptr, sigma: float, inv_c_out_sq: float, loss_weight: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the per-graph losses of the denoised ``xhat [N, 3]`` against the clean, centred ``x [N, 3]`` on the current stream; returns
    ``[W, 3]`` float32: raw_coordinate_loss = mean_i |xhat_i - x_i|^2, scaled_rmsd = mean_i |xhat_i - x_i| / (sigma sqrt 3),
    coordinate_loss = raw loss_weight_g inv_c_out_sq (``loss_weight [W]`` float32, default ones).  Tensors on the CPU take the host
    mirror.  See ``jamun_denoise_loss``."""
    x = _coords("x", x)
    N, dev = int(x.shape[0]), x.device
    xhat = _coords("xhat", xhat, dev, N)
    p = _check_ptr(ptr, N)
    s = _check_sigma(sigma)
    W = p.size - 1
    if loss_weight is not None:
        if (not torch.is_tensor(loss_weight) or loss_weight.device != dev or loss_weight.dtype != torch.float32 or tuple(loss_weight.shape) != (W,)
                or not loss_weight.is_contiguous()):
            raise RuntimeError(f"loss_weight must be a contiguous float32 [{W}] tensor on {dev}, got {getattr(loss_weight, 'dtype', None)} "
                               f"{tuple(getattr(loss_weight, 'shape', ()))} on {getattr(loss_weight, 'device', None)}")
    k = float(inv_c_out_sq)
    if not math.isfinite(k):
        raise RuntimeError(f"inv_c_out_sq must be finite, got {k}")
    out = _result("out", out, (W, 3), torch.float32, dev)
    if not x.is_cuda:
        out.copy_(torch.from_numpy(denoise_loss_host(xhat, x, p, s, k, loss_weight)))
        return out
    if W == 0:
        return out
    if N == 0:
        return out.zero_()
    _call(dev, "jamun_denoise_loss", _ptr(xhat), _ptr(x), _ptr(_device_ptr(ptr, p, dev)), W, N, C.c_float(s), _ptr(loss_weight), C.c_float(k), _ptr(out))
    return out
