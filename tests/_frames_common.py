"""What the tests of the frame-analysis layer share (trajectory encoders, superposition, internal coordinates, Ramachandran histograms,
chemical validity): the device, output buffers between sentinel pads, a chain as the callbacks see it, the stub dataset and sampler the
callbacks are driven with, and the bytes of a tree of files."""
import os

import numpy as np
import torch


def _dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda", 0)


def guarded(shape, dev, dtype, sentinel, pad: int = 64):
    """(big, out): ``out`` of ``shape`` is a view of the middle of ``big``, which holds ``pad`` sentinels in front of it and behind it."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=dev)
    return big, big[pad : pad + n].view(*shape)


def intact(big, sentinel, pad: int = 64) -> bool:
    """Whether both pads of `guarded`'s ``big`` still hold the sentinel."""
    return bool((big[:pad] == sentinel).all().item() and (big[-pad:] == sentinel).all().item())


def chain_view(frames: np.ndarray, dev, fill=float("nan")) -> torch.Tensor:
    """``frames`` [T, n, 3] as the callback sees a chain: ``block[1].transpose(0, 1)`` of a 3-chain [chains, n, T, 3] block (no copy)."""
    T, n, _ = frames.shape
    block = torch.full((3, n, T, 3), fill, dtype=torch.float32, device=dev)
    block[1] = torch.from_numpy(np.array(np.transpose(frames, (1, 0, 2)), order="C")).to(dev)  # (a writable copy)
    view = block[1].transpose(0, 1)
    assert view.shape == (T, n, 3) and view.data_ptr() == block[1].data_ptr()
    return view


class CaseDataset:
    def __init__(self, mol, label):
        self.molecule, self._label = mol, label

    def label(self):
        return self._label


class _Fabric:
    def __init__(self, device):
        self.device = device
        self.logged = []

    def log_dict(self, d):
        self.logged.append(dict(d))


class StubSampler:
    """The sampler a `TrajectoryMetricCallback` needs: ``fabric.device``, ``fabric.log_dict`` (kept in ``logged``)."""

    is_global_zero = True
    world_size = 1
    global_step = 0

    def __init__(self, device):
        self.device = device
        self.fabric = _Fabric(device)


def run(cb, batches, sampler):
    cb.on_sample_start(sampler)
    for b in batches:
        cb.on_after_sample_batch(b, sampler)
        if hasattr(cb, "flush"):
            cb.flush()
    cb.on_sample_end(sampler)
    return cb


def meter_run(callback, root, mol, batches, sampler_device, xyz=None, **kw):
    """One run of a metric callback (``kw``: its arguments) on a dataset ``"m"`` of ``mol``, with frames of its own if ``xyz``, under a
    sampler on ``sampler_device`` -> (callback, sampler)."""
    ds = CaseDataset(mol, "m")
    if xyz is not None:
        ds.xyz = xyz
    cb = callback([ds], output_dir=str(root), **kw)
    smp = StubSampler(sampler_device)
    run(cb, batches, smp)
    return cb, smp


def tree(root: str) -> dict:
    """relative path -> bytes of every file under ``root``."""
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out
