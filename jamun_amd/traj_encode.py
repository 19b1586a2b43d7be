"""Device-side encoding of trajectory files for ``SaveTrajectoryCallback`` (``jamun_traj.hip``).

The frames of a batch are on the GPU when the callback gets them; the ``.pdb`` text and the ``.dcd`` records are produced there
(``jamun_encode_pdb_models`` / ``jamun_encode_dcd_frames``) and reach the files in chunks of frames through FIXED staging memory:
one device buffer and two page-locked host buffers of ``STAGING_BYTES`` each, whatever the number of frames or chains — a
20 000-step batch of 256 dipeptides is ~9 GB of PDB text and is never resident.  While one page-locked buffer is written to the
file, the next chunk is encoded and copied into the other.  All device work runs on ONE side stream (the walk keeps the
current one).  `pdb.save_pdb` / `pdb.save_dcd` remain the specification of the bytes and the fallback.

With ``SaveTrajectoryCallback(superpose=True)`` the frames are superposed on the reference structure on the same stream, in front of
the encoders (``jamun_superpose_frames``), into ONE more device buffer of ``STAGING_BYTES`` that exists only then: a chain goes through
it in chunks of ``align_frames_per_chunk`` frames (32 MiB hold 96 000 frames of a 29-atom molecule: a 20 000-frame chain is one chunk),
each chunk aligned once and read by the encoders of all its files.  The RMSD of a chunk leaves through the staging buffers like any
encoded chunk.  The memory is fixed whatever the number of frames: `staging_bytes` reports it.

With ``SaveTrajectoryCallback(torsions=...)`` one more job per chunk of ``features_frames_per_chunk`` frames computes the torsion angles of
the RAW frames (``jamun_internal_coords``: internal coordinates do not change under superposition) straight into the device staging
buffer, behind the same event on the same stream; the sink copies the chunk into the chain's ``[T, F]`` array.  No buffer is added: the
index table (16 bytes per torsion, uploaded once per label by the callback) is all the device memory the option costs.
"""

from __future__ import annotations

from typing import Callable, Dict, Iterable, Tuple

import torch

from . import native
from .pdb import pdb_model_template

STAGING_BYTES = 32 << 20  # per buffer (a power of two: PyTorch's pinned allocator rounds up to one)


class DeviceTrajectoryEncoder:
    def __init__(self, device: torch.device):
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.Stream(self.device)
            self._dev = torch.empty(STAGING_BYTES, dtype=torch.uint8, device=self.device)
            self._pinned = [torch.empty(STAGING_BYTES, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._events = [torch.cuda.Event() for _ in range(2)]
            self._counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._host = [p.numpy() for p in self._pinned]
        self._templates: Dict[int, Tuple[dict, torch.Tensor, torch.Tensor]] = {}
        self._aligned = None  # float32 scratch of STAGING_BYTES for superposed frames, allocated with the first `align_view`

    def staging_bytes(self) -> int:
        """Bytes of staging memory this encoder holds (device + page-locked)."""
        return int(self._dev.numel() + sum(p.numel() for p in self._pinned) + (4 * self._aligned.numel() if self._aligned is not None else 0))

    def template(self, mol: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """`pdb.pdb_model_template` of ``mol`` on the device, built once per molecule."""
        hit = self._templates.get(id(mol))
        if hit is None or hit[0] is not mol:
            body, off = pdb_model_template(mol)
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                hit = (mol, torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device), torch.from_numpy(off).to(self.device))
            self.stream.synchronize()
            self._templates[id(mol)] = hit
        return hit[1], hit[2]

    def reset_unencodable(self) -> None:
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self._counter.zero_()

    def unencodable(self) -> int:
        """Values counted since `reset_unencodable` (waits for the side stream)."""
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            return int(self._counter.item())

    def pdb_frames_per_chunk(self, body_len: int) -> int:
        return STAGING_BYTES // (14 + 16 + body_len)  # (a MODEL line never exceeds 14 + 16 characters, native.pdb_models_nbytes)

    @staticmethod
    def dcd_frames_per_chunk(n_atoms: int) -> int:
        return STAGING_BYTES // (3 * (4 * n_atoms + 8))

    def encode_pdb(self, frames: torch.Tensor, first_model: int, body: torch.Tensor, coord_off: torch.Tensor) -> Callable[[torch.Tensor], int]:
        return lambda out: native.encode_pdb_models(frames, first_model, body, coord_off, out, self._counter)

    @staticmethod
    def encode_dcd(frames: torch.Tensor) -> Callable[[torch.Tensor], int]:
        return lambda out: native.encode_dcd_frames(frames, out)

    @staticmethod
    def align_frames_per_chunk(n_atoms: int) -> int:
        """Frames of ``n_atoms`` atoms the scratch of `align_view` holds (and whose RMSD, 4 bytes each, fits a staging buffer)."""
        return min(STAGING_BYTES // (12 * n_atoms), STAGING_BYTES // 4) if n_atoms > 0 else 0

    def align_view(self, n_atoms: int, n_frames: int) -> torch.Tensor:
        """A ``[n_frames, n_atoms, 3]`` view of the scratch for superposed frames, laid out like a chain (``[n, T, 3]``: the frames of an
        atom adjacent, so one lane per frame writes and reads it coalesced)."""
        if self._aligned is None:
            with torch.cuda.device(self.device):
                self._aligned = torch.empty(STAGING_BYTES // 4, dtype=torch.float32, device=self.device)
        if 3 * n_atoms * n_frames > self._aligned.numel():
            raise RuntimeError(f"{n_frames} frames of {n_atoms} atoms do not fit the {4 * self._aligned.numel()}-byte scratch")
        return self._aligned[: 3 * n_atoms * n_frames].view(n_atoms, n_frames, 3).transpose(0, 1)

    @staticmethod
    def superpose(frames: torch.Tensor, ref: torch.Tensor, aligned: torch.Tensor) -> Callable[[torch.Tensor], int]:
        """A job for `run`: ``frames`` superposed on ``ref`` into ``aligned`` (a view of `align_view`); the job's bytes are the float32
        RMSD of the frames."""
        k = int(frames.shape[0])
        return lambda out: (native.superpose_frames(frames, ref, out=aligned, rmsd=out[: 4 * k].view(torch.float32)), 4 * k)[1]

    @staticmethod
    def features_frames_per_chunk(width: int) -> int:
        """Frames whose ``width`` float32 internal coordinates fit a staging buffer."""
        return STAGING_BYTES // (4 * width) if width > 0 else 0

    @staticmethod
    def features(frames: torch.Tensor, index_dev: torch.Tensor, cossin: bool = False) -> Callable[[torch.Tensor], int]:
        """A job for `run`: the internal coordinates of ``frames`` for the table ``index_dev`` (int32 [F, 4], on the device), written by the
        kernel into the staging buffer itself; the job's bytes are the float32 ``[frames, W]`` block, W = F or 2 F."""
        k, w = int(frames.shape[0]), int(index_dev.shape[0]) * (2 if cossin else 1)
        return lambda out: (native.internal_coords(frames, index_dev, cossin=cossin, out=out[: 4 * k * w].view(torch.float32).view(k, w)), 4 * k * w)[1]

    def run(self, jobs: Iterable[Tuple[Callable[[torch.Tensor], int], Callable[[memoryview], None]]]) -> None:
        """``jobs``: (encode, sink) pairs, one per chunk.  ``encode(out)`` queues a kernel that fills the device staging buffer and
        returns the byte count; ``sink(bytes)`` gets those bytes from a page-locked buffer once their copy has landed — while the
        next job's kernel and copy are already queued into the other buffer."""
        pending = None
        slot = 0
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            for encode, sink in jobs:
                nbytes = encode(self._dev)
                if nbytes > STAGING_BYTES:
                    raise RuntimeError(f"a chunk of {nbytes} bytes does not fit the {STAGING_BYTES}-byte staging buffer")
                self._pinned[slot][:nbytes].copy_(self._dev[:nbytes], non_blocking=True)  # (stream order keeps the next kernel behind this copy)
                self._events[slot].record(self.stream)
                if pending is not None:
                    self._drain(*pending)
                pending = (slot, nbytes, sink)
                slot ^= 1
            if pending is not None:
                self._drain(*pending)

    def _drain(self, slot: int, nbytes: int, sink) -> None:
        self._events[slot].synchronize()
        sink(memoryview(self._host[slot])[:nbytes])
