"""What the five per-trajectory meters (`ramachandran.RamachandranMetrics`, `validity.ChemicalValidityMetrics`, `tica.TICAMetrics`,
`msm.MSMMetrics`, `swd.SlicedWassersteinMetrics`) share: the ``TrajectoryMetric`` protocol `callbacks.TrajectoryMetricCallback` drives, the choice between the device and the host path, the reference frames, the view of a
chain, and the reproducible ``.npz`` writer.  A meter derives from `TrajectoryMeter`, names its directory and its device condition, and
keeps its own tables, ``on_sample_start``, the body of ``update`` and ``compute``."""

from __future__ import annotations

import os
import zipfile
from typing import Optional, Tuple

import numpy as np
import torch


def save_npz(path: str, **arrays) -> None:
    """``np.savez`` with a fixed time stamp in the archive: the same arrays give the same bytes (``np.load`` reads it as any ``.npz``)."""
    tmp = path + ".tmp"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o600 << 16
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(a), allow_pickle=False)
    os.replace(tmp, path)


class TrajectoryMeter:
    """The meter of one dataset.  A subclass sets `DIRECTORY` and defines `_device_fits` and `_device_needs`."""

    DIRECTORY = ""  # files go under <output_dir>/<label>/<DIRECTORY>/ on rank 0

    def __init__(self, dataset, sample_key: str, output_dir: str, device: str):
        if device not in ("auto", "host", "device"):
            raise ValueError(f"device must be 'auto', 'host' or 'device', got {device!r}")
        self.dataset = dataset
        self.label = dataset.label()
        self.sample_key = sample_key
        self.output_dir = output_dir
        self.mode = device
        self.torch_device: Optional[torch.device] = None
        self._dev: dict = {}  # device -> the meter's tables uploaded once
        self.num_chains_seen = 0
        self.joined_frames = 0
        self._pending: list = []

    def _device_fits(self) -> bool:
        """Whether the kernels take this meter's problem (float32 tensors on a GPU and a library that loads are asked here)."""
        raise NotImplementedError

    def _device_needs(self) -> str:
        """The text of the error ``device='device'`` raises where the device path is not to be had."""
        raise NotImplementedError

    # ---- protocol ------------------------------------------------------------------------------------------------------------------------

    def to(self, device):
        self.torch_device = torch.device(device) if device is not None else None
        return self

    def on_after_sample_batch(self) -> None:
        pass

    def on_sample_end(self) -> None:
        if self._pending:
            self.compute()

    # ---- for the subclasses --------------------------------------------------------------------------------------------------------------

    def _is_rank_zero(self) -> bool:
        from . import dist

        return dist.rank_world()[0] == 0

    def _dir(self) -> str:
        d = os.path.join(self.output_dir, self.label, self.DIRECTORY)
        os.makedirs(d, exist_ok=True)
        return d

    def _device_path(self, t) -> bool:
        """Whether frames ``t`` (a tensor or an array) go through the kernels."""
        if self.mode == "host":
            return False
        ok = torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and self._device_fits()
        if ok:
            from . import _lib

            if not _lib.available():
                if self.mode == "device":
                    _lib.load()  # (raises the loader's own error)
                ok = False
        if not ok and self.mode == "device":
            raise RuntimeError(self._device_needs())
        return ok

    def _reference_frames(self, n_atoms: int, what: str, ref=None):
        """The frames the samples are judged against as a tensor ``[T, n_atoms, 3]``, or None: ``ref`` (frames, or the path of an ``.npy``
        of them) if given, else the dataset's own ``xyz``.  ``what`` begins the error for frames of another shape."""
        if ref is None:
            ref = getattr(self.dataset, "xyz", None)
        if ref is None:
            return None
        if isinstance(ref, (str, os.PathLike)):
            ref = np.load(ref)
        if not torch.is_tensor(ref):
            ref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32))
        if ref.ndim != 3 or ref.shape[2] != 3 or ref.shape[1] != n_atoms:
            raise ValueError(f"{what} {self.label!r} must have shape [T, {n_atoms}, 3], got {tuple(ref.shape)}")
        return ref if ref.shape[0] > 0 else None

    def _on_compute_device(self, chunk: torch.Tensor) -> torch.Tensor:
        """Reference frames where they are counted: on the meter's GPU (`to`) if the device path can take them, else on the host."""
        use_gpu = (self.mode != "host" and self.torch_device is not None and self.torch_device.type == "cuda" and chunk.dtype == torch.float32
                   and self._device_fits())
        if use_gpu and not chunk.is_cuda:
            chunk = chunk.to(self.torch_device)
        elif not use_gpu and chunk.is_cuda:
            chunk = chunk.cpu()
        return chunk

    def _next_chain(self, sample) -> Tuple[int, object, int]:
        """The head of ``update``: ``(the chain's running index, its frames [T, n, 3] as a view of the RAW chain, the frames joined before
        it)``.  The caller adds the chain's frames to ``joined_frames``."""
        x = sample[self.sample_key]
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"Invalid sample shape: {tuple(x.shape)}, expected (num_atoms, num_frames, 3).")
        index = self.num_chains_seen
        self.num_chains_seen += 1
        frames = x.transpose(0, 1) if torch.is_tensor(x) else np.transpose(np.asarray(x), (1, 0, 2))
        return index, frames, self.joined_frames

    def _take_pending(self) -> Tuple[list, bool, Optional[str]]:
        """The head of ``compute``: ``(the records since the last call, whether this rank writes, the directory if there is something to write)``."""
        pending, self._pending = self._pending, []
        write = self._is_rank_zero()
        return pending, write, self._dir() if write and pending else None
