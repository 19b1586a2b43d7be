"""The calls that encode or analyse frames of a trajectory and never touch a sampler: the binding of ``csrc/jamun_frames.cpp``, as
`native` is the binding of ``csrc/jamun_api.cpp`` (which hands out this module's public names too).  One section per kernel family, in
the order of the C file; what the sections share comes first.  Every argument is checked before the library or a GPU is needed wherever
the check needs neither, and ``tests/golden/frames_refusals.json`` pins the class and the text of those refusals.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib


# ---- what the calls below share -------------------------------------------------------------------------------------------------------

def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


def _call(device, fn_name: str, *args) -> None:
    """Queue ``fn_name`` of the library on the current stream of ``device``: the stream is appended to ``args``, a refusal is a
    ``RuntimeError`` with the library's text."""
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(getattr(lib, fn_name)(*args, _stream()))


def _result(name: str, given: Optional[torch.Tensor], shape: tuple, dtype: torch.dtype, device, fill=None) -> torch.Tensor:
    """The tensor a result is written to: ``given`` if it is a contiguous ``dtype`` tensor of ``shape`` on ``device`` (``RuntimeError``
    otherwise), else a new one, holding ``fill`` where the call may write nothing."""
    if given is None:
        return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)
    if given.device != device or given.dtype != dtype or tuple(given.shape) != tuple(shape) or not given.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on {device}, "
                           f"got {given.dtype} {tuple(given.shape)} on {given.device}")
    return given


def _on_device(table) -> bool:
    return torch.is_tensor(table) and table.is_cuda


def _table(what: str, spec: str, table, on_device: bool, device, dtype: torch.dtype, shape: tuple) -> torch.Tensor:
    """A table of indices or thresholds as a tensor on ``device``.  A host table (an array its ``check_*`` function returned) is uploaded;
    one handed in on the device is taken as checked once it is a contiguous ``dtype`` tensor of ``shape`` there (``None``: any length),
    ``ValueError`` otherwise.  ``spec`` is how the message words type and shape."""
    if not on_device:
        return torch.from_numpy(table).to(device)
    if (not torch.is_tensor(table) or table.device != device or table.dtype != dtype or table.ndim != len(shape) or not table.is_contiguous()
            or any(want is not None and want != have for want, have in zip(shape, table.shape))):
        raise ValueError(f"{what} on the device must be a contiguous {spec} tensor on {device}, got {getattr(table, 'dtype', None)} "
                         f"{tuple(getattr(table, 'shape', ()))} on {getattr(table, 'device', None)}")
    return table


def _fit_31_bits(text: str, *counts: int) -> None:
    """``RuntimeError(text)`` if one of ``counts`` is more than the C entries' int32 arguments hold."""
    if any(c > 0x7FFFFFFF for c in counts):
        raise RuntimeError(text)


_LONG_AXIS = {"columns": (0, "frames"), "keys": (1, "keys")}  # what a row holds -> (the axis that may be long, what it counts)


def _rows(name: str, a: torch.Tensor, dtype: torch.dtype, noun: str, device=None) -> int:
    """``RuntimeError`` unless ``a [R, W]`` is a ``dtype`` tensor on a GPU (``device`` if given) whose rows hold their ``W`` ``noun`` (a key
    of `_LONG_AXIS`) adjacent, at least ``W`` apart, and whose long axis fits 31 bits; returns the row stride in elements."""
    R, W = int(a.shape[0]), int(a.shape[1])
    if (not a.is_cuda or a.dtype != dtype or (W > 1 and a.stride(1) != 1) or (R > 1 and a.stride(0) < W)
            or (device is not None and a.device != device)):
        raise RuntimeError(f"{name} must be a {str(dtype).replace('torch.', '')} tensor on the GPU{'' if device is None else f' ({device})'} with "
                           f"adjacent {noun}, got {a.dtype} {tuple(a.shape)} strides {tuple(a.stride())} on {a.device}")
    axis, unit = _LONG_AXIS[noun]
    _fit_31_bits(f"{a.shape[axis]} {unit}: the count must fit 31 bits", int(a.shape[axis]))
    return int(a.stride(0)) if R > 1 else W


def _dense(name: str, a, dtype: torch.dtype, device=None, convert: bool = True) -> torch.Tensor:
    """A dense table as a contiguous ``dtype`` tensor on ``device`` (``None``: where it is, for a caller that has checks of its own to
    make before the upload).  A host array becomes a tensor, converted to ``dtype`` on the way unless ``convert`` is off; a tensor, on the
    device or on the host, is used as it is.  What then does not hold ``dtype`` is a ``ValueError``."""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.dtype(str(dtype).replace("torch.", "")) if convert else None))
    if a.dtype != dtype:
        raise ValueError(f"{name} must hold {str(dtype).replace('torch.', '')}, got {a.dtype}")
    return (a if device is None else a.to(device)).contiguous()


_work: Dict[Tuple[str, int], torch.Tensor] = {}  # (device, stream) -> the workspace of the two-pass reductions, grown on demand


def _workspace(device, n_doubles: int) -> torch.Tensor:
    """The workspace on the current stream of ``device`` that every family shares (the TICA and k-means reductions, the merge passes of
    the segment sort, the quantile integral): one per (device, stream), since the calls of one stream run one after the other and those
    of two streams may not share partial sums."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    have = _work.get(key)
    if have is None or have.numel() < n_doubles:
        have = _work[key] = torch.empty(max(int(n_doubles), 1), dtype=torch.float64, device=device)
    return have


def _workspace_for(device, query: str, *args, dtype: torch.dtype = torch.float64) -> Tuple[int, int]:
    """``(pointer, capacity)`` of the shared workspace, grown to what the library's ``query`` (a ``*_work`` entry) asks for ``args``, in
    elements of ``dtype``: the doubles themselves, or a float32 view of them for the segment sort, which counts in floats."""
    need = C.c_int64()
    _lib.check(getattr(_lib.load(), query)(*args, C.byref(need)))
    work = _workspace(device, need.value) if dtype == torch.float64 else _workspace(device, (need.value + 1) // 2).view(dtype)
    return _ptr(work), int(work.numel())


# ---- trajectory file encoders (jamun_traj.hip) ---------------------------------------------------------------------------------------

def pdb_models_nbytes(body_len: int, first_model: int, n_frames: int) -> int:
    """Exact size of PDB models ``first_model .. first_model + n_frames - 1`` with a body of ``body_len`` bytes (host only)."""
    lib = _lib.load()
    out = C.c_int64()
    _lib.check(lib.jamun_pdb_models_nbytes(int(body_len), int(first_model), int(n_frames), C.byref(out)))
    return int(out.value)


def _frame_strides(xyz: torch.Tensor) -> Tuple[int, int, int, int]:
    """``xyz [T, n, 3]`` (any strides over T and n, components adjacent) -> (frame stride, atom stride, n, T) in floats: no copy."""
    if not xyz.is_cuda or xyz.dtype != torch.float32 or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise RuntimeError(f"frames must be a float32 [frames, atoms, 3] tensor on the GPU, got {xyz.dtype} {tuple(xyz.shape)} on {xyz.device}")
    if xyz.shape[0] > 0 and xyz.shape[1] > 0 and xyz.stride(2) != 1:
        raise RuntimeError("the three components of an atom must be adjacent in memory")
    return int(xyz.stride(0)), int(xyz.stride(1)), int(xyz.shape[1]), int(xyz.shape[0])


def encode_pdb_models(xyz: torch.Tensor, first_model: int, body: torch.Tensor, coord_off: torch.Tensor, out: torch.Tensor,
                      unencodable: torch.Tensor) -> int:
    """Queue the text of PDB models ``first_model ...`` of the frames ``xyz [T, n, 3]`` (device fp32, nm, a view of either trajectory
    layout) into ``out`` (device uint8) on the current stream; returns the number of bytes.  ``body`` (uint8) / ``coord_off`` (int32)
    are `pdb.pdb_model_template` on the device; ``unencodable`` (one int32, zeroed by the caller) counts the values the fixed
    layout cannot hold.  See ``jamun_encode_pdb_models``."""
    _lib.load()  # (here and below: a missing library is reported at the point where it always was, among the other refusals; `_call` finds it loaded)
    fs, as_, n, T = _frame_strides(xyz)
    need = pdb_models_nbytes(body.numel(), first_model, T)
    _call(xyz.device, "jamun_encode_pdb_models", _ptr(xyz), fs, as_, n, T, int(first_model), _ptr(body), int(body.numel()), _ptr(coord_off), _ptr(out),
          int(out.numel()), _ptr(unencodable))
    return need


def encode_dcd_frames(xyz: torch.Tensor, out: torch.Tensor) -> int:
    """Queue the DCD coordinate records of the frames ``xyz [T, n, 3]`` into ``out`` (device uint8) on the current stream; returns the
    number of bytes.  See ``jamun_encode_dcd_frames``."""
    _lib.load()
    fs, as_, n, T = _frame_strides(xyz)
    _call(xyz.device, "jamun_encode_dcd_frames", _ptr(xyz), fs, as_, n, T, _ptr(out), int(out.numel()))
    return T * 3 * (4 * n + 8)


# ---- superposition (jamun_superpose.hip) ----------------------------------------------------------------------------------------------

def superpose_frames(frames: torch.Tensor, ref: torch.Tensor, out: Optional[torch.Tensor] = None, rmsd: Optional[torch.Tensor] = None,
                     want_rmsd: bool = True):
    """Queue the superposition of the frames ``frames [T, n, 3]`` (device fp32, a view of either trajectory layout) on ``ref [n, 3]`` on
    the current stream: returns ``(aligned [T, n, 3], rmsd [T])``, each frame rotated (properly) and translated onto ``ref`` with the
    least RMSD, and that RMSD.  ``out`` receives the aligned frames (default: a new tensor with the layout of ``frames``); it may be
    ``frames`` itself.  ``rmsd`` (contiguous float32 [T]) receives the RMSD (default: a new tensor); ``want_rmsd=False`` passes no RMSD
    buffer and returns ``None`` for it.  See ``jamun_superpose_frames``."""
    _lib.load()
    fs, as_, n, T = _frame_strides(frames)
    _fit_31_bits(f"{T} frames of {n} atoms: both counts must fit 31 bits", n, T)
    if not ref.is_cuda or ref.device != frames.device or ref.dtype != torch.float32 or tuple(ref.shape) != (n, 3):
        raise RuntimeError(f"ref must be a float32 [{n}, 3] tensor on {frames.device}, got {ref.dtype} {tuple(ref.shape)} on {ref.device}")
    ref = ref.contiguous()
    if out is None:
        out = torch.empty_like(frames)  # (keeps the strides of a dense view such as a transposed chain)
    if out.device != frames.device or tuple(out.shape) != tuple(frames.shape):  # (a strided view: not `_result`'s contiguous tensor)
        raise RuntimeError(f"out must be a [{T}, {n}, 3] tensor on {frames.device}, got {tuple(out.shape)} on {out.device}")
    ofs, oas, _, _ = _frame_strides(out)
    if not want_rmsd:
        rmsd = None
    elif rmsd is None:
        rmsd = torch.empty(T, dtype=torch.float32, device=frames.device)
    elif rmsd.device != frames.device or rmsd.dtype != torch.float32 or tuple(rmsd.shape) != (T,) or not rmsd.is_contiguous():
        raise RuntimeError(f"rmsd must be a contiguous float32 [{T}] tensor on {frames.device}")  # (its own text: no "got")
    if rmsd is not None and n == 0:
        rmsd.zero_()  # (frames without atoms: the call writes nothing)
    _call(frames.device, "jamun_superpose_frames", _ptr(frames), fs, as_, n, T, _ptr(ref), _ptr(out), ofs, oas, _ptr(rmsd))
    return out, rmsd


# ---- internal coordinates (jamun_intcoord.hip) ----------------------------------------------------------------------------------------

INTCOORD_FEATURE_TILE = 16  # table rows a workgroup of k_internal_coords stages at a time (JAMUN_INTCOORD_FTILE, jamun_internal.h)


def check_index_table(index, n_atoms: int) -> np.ndarray:
    """The feature table of `internal_coords` checked on the host: an integer ``[F, 4]`` array (or tensor) whose rows are 2 to 4 atom
    indices in ``[0, n_atoms)`` followed by ``-1`` up to four entries.  Returns it as contiguous int32; anything else is a ``ValueError``."""
    if torch.is_tensor(index):
        if index.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise ValueError(f"the index table must hold integers, got {index.dtype}")
        a = index.detach().cpu().numpy()
    else:
        a = np.asarray(index)
        if a.dtype.kind not in "iu":
            raise ValueError(f"the index table must hold integers, got {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"the index table must have shape [F, 4], got {tuple(a.shape)}")
    a = a.astype(np.int64)
    valid = a >= 0
    k = np.cumprod(valid, axis=1).sum(axis=1)  # leading non-negative entries of each row
    tail = np.arange(4)[None, :] >= k[:, None]
    bad = (k < 2) | ((a != -1) & tail).any(axis=1) | ((a >= n_atoms) & ~tail).any(axis=1)
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError(f"row {j} of the index table, {a[j].tolist()}, is not 2 to 4 atom indices in [0, {n_atoms}) followed by -1")
    return np.ascontiguousarray(a, dtype=np.int32)


def internal_coords(frames: torch.Tensor, index, cossin: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the internal coordinates of the frames ``frames [T, n, 3]`` (device fp32, a view of either trajectory layout) on the current
    stream: float32 ``[T, F]``, or ``[T, 2 F]`` interleaved (cos, sin) pairs with ``cossin`` (a distance as (d, 0)).  ``index [F, 4]``: per
    row 2 (distance, nm), 3 (bond angle) or 4 (dihedral, mdtraj's sign) atom indices, then ``-1``.  A host table (array, list, CPU tensor) is
    checked by `check_index_table` and uploaded; an int32 tensor already on the device of ``frames`` is taken as checked (upload once,
    call often: the kernel answers an index out of range with NaN, it never reads there).  ``out`` (contiguous float32 of that shape on
    the device) receives the result; default a new tensor.  See ``jamun_internal_coords``."""
    if not torch.is_tensor(frames) or frames.ndim != 3 or frames.shape[2] != 3:
        raise RuntimeError(f"frames must be a [frames, atoms, 3] tensor, got {tuple(getattr(frames, 'shape', ()))}")
    on_device = _on_device(index)
    if not on_device:
        index = check_index_table(index, int(frames.shape[1]))  # (before anything needs a GPU)
    fs, as_, n, T = _frame_strides(frames)
    F = int(index.shape[0])
    _fit_31_bits(f"{T} frames of {n} atoms, {F} features: the counts must fit 31 bits", n, T, F)
    _lib.load()
    index = _table("an index table", "int32 [F, 4]", index, on_device, frames.device, torch.int32, (None, 4))
    W = 2 * F if cossin else F
    out = _result("out", out, (T, W), torch.float32, frames.device)
    _call(frames.device, "jamun_internal_coords", _ptr(frames), fs, as_, n, T, _ptr(index), F, 1 if cossin else 0, _ptr(out), int(out.numel()))
    return out


# ---- histograms of angle pairs and their Jensen-Shannon divergence (jamun_hist.hip) -------------------------------------------------------

HIST_SLICE = 4096    # frames of a segment one workgroup of k_hist2d_pairs counts (JAMUN_HIST_SLICE, jamun_internal.h)
HIST_MAX_BINS = 128  # bins per axis the kernel takes (JAMUN_HIST_MAX_BINS: 128 * 128 counters are 64 KB of LDS)
HIST_MAX_CUTS = 64   # JAMUN_HIST_MAX_CUTS

_hist_edges: Dict[Tuple[str, int], torch.Tensor] = {}  # (device, bins) -> the uploaded edges


def hist_edges(bins: int) -> np.ndarray:
    """The bin edges of both axes, float64 ``[bins + 1]``: what ``np.histogram2d(..., bins, range=((-pi, pi), (-pi, pi)))`` uses."""
    return np.linspace(-np.pi, np.pi, int(bins) + 1)


def check_cuts(cuts, n_frames: int) -> np.ndarray:
    """The rule of the cuts, for `ramachandran.histogram_host` and `hist2d_pairs` alike: 1 to 64 integers ascending strictly within
    ``[1, n_frames]`` (``ValueError`` otherwise), returned as int64.  Host only."""
    c = np.asarray(cuts.detach().cpu().numpy() if torch.is_tensor(cuts) else cuts)
    if c.ndim != 1 or c.dtype.kind not in "iu" or not 1 <= c.shape[0] <= HIST_MAX_CUTS:
        raise ValueError(f"cuts must be 1 to {HIST_MAX_CUTS} integers, got {c.dtype} {tuple(c.shape)}")
    c = c.astype(np.int64)
    if c[0] < 1 or c[-1] > n_frames or (np.diff(c) <= 0).any():
        raise ValueError(f"cuts must ascend strictly within [1, {n_frames}], got {c.tolist()}")
    return c


def check_hist_args(n_frames: int, width: int, pairs, bins, cuts) -> Tuple[Optional[np.ndarray], int, np.ndarray]:
    """The arguments of `hist2d_pairs` checked on the host; ``ValueError`` for: ``pairs`` not an integer ``[P, 2]`` table of columns in
    ``[0, width)`` (``None`` stands for a table already on the device, taken as checked), ``bins`` not an integer in ``[1, 128]``,
    ``cuts`` not 1 to 64 integers ascending strictly within ``[1, n_frames]``.  Returns ``(pairs int32 [P, 2] or None, bins, cuts int32 [C])``."""
    if pairs is not None:
        a = pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else np.asarray(pairs)
        if a.size == 0:
            a = a.reshape(-1, 2).astype(np.int64)
        if a.dtype.kind not in "iu":
            raise ValueError(f"pairs must hold integers, got {a.dtype}")
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"pairs must have shape [P, 2], got {tuple(a.shape)}")
        a = a.astype(np.int64)
        bad = ((a < 0) | (a >= width)).any(axis=1)
        if bad.any():
            j = int(np.flatnonzero(bad)[0])
            raise ValueError(f"row {j} of pairs, {a[j].tolist()}, is not two columns in [0, {width})")
        pairs = np.ascontiguousarray(a, dtype=np.int32)
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= HIST_MAX_BINS:
        raise ValueError(f"bins must be an integer in [1, {HIST_MAX_BINS}], got {bins!r}")
    return pairs, int(bins), np.ascontiguousarray(check_cuts(cuts, n_frames), dtype=np.int32)


def hist2d_pairs(angles: torch.Tensor, pairs, bins: int, cuts, out: Optional[torch.Tensor] = None,
                 skipped: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Queue the segment histograms of ``angles [T, W]`` (device fp32 with adjacent columns: what `internal_coords` returns, or a view of
    it with a row stride) on the current stream: ``(counts uint32-valued int32 [C, P, bins, bins], skipped int32 [C, P])``; segment ``c``
    holds the frames ``cuts[c-1] <= t < cuts[c]``.  The rule of every bin is `ramachandran.histogram_host`'s, integer for integer.
    ``pairs [P, 2]`` (x column, y column): a host table is checked and uploaded, an int32 tensor on the device of ``angles`` is taken as
    checked (a column out of range there counts nothing).  The arguments are checked before anything needs a GPU (`check_hist_args`).
    ``out`` / ``skipped`` (contiguous int32 of those shapes on the device) receive the result; default new tensors.  The counters are
    unsigned 32-bit; torch has no arithmetic for that type, so they are handed out as int32 (a segment has fewer than 2^31 frames).
    See ``jamun_hist2d_pairs``."""
    if not torch.is_tensor(angles) or angles.ndim != 2:
        raise ValueError(f"angles must be a [frames, width] tensor, got {tuple(getattr(angles, 'shape', ()))}")
    T, W = int(angles.shape[0]), int(angles.shape[1])
    on_device = _on_device(pairs)
    host_pairs, bins, cuts = check_hist_args(T, W, None if on_device else pairs, bins, cuts)
    row_stride = _rows("angles", angles, torch.float32, "columns")
    _lib.load()
    dev = angles.device
    pairs = _table("a pairs table", "int32 [P, 2]", pairs if on_device else host_pairs, on_device, dev, torch.int32, (None, 2))
    P, C = int(pairs.shape[0]), int(cuts.shape[0])
    key = (str(dev), bins)
    if key not in _hist_edges:
        _hist_edges[key] = torch.from_numpy(hist_edges(bins)).to(dev)
    edges = _hist_edges[key]
    out = _result("out", out, (C, P, bins, bins), torch.int32, dev)
    skipped = _result("skipped", skipped, (C, P), torch.int32, dev)
    _call(dev, "jamun_hist2d_pairs", _ptr(angles), row_stride, T, W, _ptr(pairs), P, _ptr(edges), bins, cuts.ctypes.data, C, _ptr(out), int(out.numel()),
          _ptr(skipped))
    return out, skipped


def js_divergence(counts: torch.Tensor, ref_counts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Queue the Jensen-Shannon divergences of the prefix sums of the segment histograms ``counts [C, P, B, B]`` (int32 on the device, as
    `hist2d_pairs` returns them) against ``ref_counts [P, B, B]`` or ``[B, B]`` (int32, same device): ``(pooled float64 [C], per_pair
    float64 [C, P])`` in nats, as `ramachandran.js_divergence_host` defines them.  A prefix or a reference without a count gives NaN
    (the host specification raises for an empty reference; nothing is read back here).  See ``jamun_js_divergence``."""
    if not torch.is_tensor(counts) or counts.ndim != 4 or counts.shape[2] != counts.shape[3] or counts.dtype != torch.int32:
        raise ValueError(f"counts must be an int32 [C, P, B, B] tensor, got {getattr(counts, 'dtype', None)} {tuple(getattr(counts, 'shape', ()))}")
    C, P, B = int(counts.shape[0]), int(counts.shape[1]), int(counts.shape[2])
    if not torch.is_tensor(ref_counts) or ref_counts.dtype != torch.int32 or tuple(ref_counts.shape) not in ((P, B, B), (B, B)):
        raise ValueError(f"ref_counts must be an int32 [{P}, {B}, {B}] or [{B}, {B}] tensor, got {getattr(ref_counts, 'dtype', None)} "
                         f"{tuple(getattr(ref_counts, 'shape', ()))}")
    if not 1 <= B <= HIST_MAX_BINS or not 1 <= C <= HIST_MAX_CUTS or P < 1:
        raise ValueError(f"{C} cuts, {P} pairs, {B} bins: at most {HIST_MAX_CUTS} cuts and {HIST_MAX_BINS} bins, and at least one of each")
    if not counts.is_cuda or ref_counts.device != counts.device or not counts.is_contiguous() or not ref_counts.is_contiguous():
        raise RuntimeError(f"counts and ref_counts must be contiguous tensors on one GPU, got {counts.device} and {ref_counts.device}")
    _lib.load()
    pooled = torch.empty((C,), dtype=torch.float64, device=counts.device)
    per_pair = torch.empty((C, P), dtype=torch.float64, device=counts.device)
    _call(counts.device, "jamun_js_divergence", _ptr(counts), C, P, B, _ptr(ref_counts), P if ref_counts.ndim == 3 else 1, _ptr(pooled), _ptr(per_pair))
    return pooled, per_pair


# ---- chemical validity of frames (jamun_validity.hip) -----------------------------------------------------------------------------------------

VALIDITY_MAX_ATOMS = 256    # atoms k_validity_frames takes (JAMUN_VALIDITY_MAX_ATOMS, jamun_internal.h)
VALIDITY_CHUNK = 64         # atoms a workgroup stages in LDS at a time (JAMUN_VALIDITY_CHUNK)
VALIDITY_SPLIT_ATOMS = 32   # above this many atoms four waves share a workgroup's frames (JAMUN_VALIDITY_SPLIT_ATOMS)

_VALIDITY_KEYS = (("clash_s", np.float32), ("bonds", np.int32), ("bond_lo_s", np.float32), ("bond_hi_s", np.float32))


def check_validity_tables(tables, n_atoms: int) -> Dict[str, np.ndarray]:
    """The tables of `validity_counts` (``clash_s`` float32 ``[n (n - 1) / 2]``, ``bonds`` integer ``[B, 2]``, ``bond_lo_s`` / ``bond_hi_s``
    float32 ``[B]``: what `validity.validity_tables` makes) checked on the host; ``ValueError`` for a wrong type or shape, a bond with an
    index outside ``[0, n_atoms)`` or a bond of an atom with itself.  Returns the four as contiguous arrays (float32 / int32)."""
    out = {}
    for key, dtype in _VALIDITY_KEYS:
        a = tables[key]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        kind = "iu" if dtype is np.int32 else "f"
        if a.dtype.kind not in kind or (kind == "f" and a.dtype != np.float32):
            raise ValueError(f"{key} must hold {'integers' if kind == 'iu' else 'float32'}, got {a.dtype}")
        out[key] = a
    pairs = n_atoms * (n_atoms - 1) // 2
    if out["clash_s"].shape != (pairs,):
        raise ValueError(f"clash_s must have shape [{pairs}] for {n_atoms} atoms, got {tuple(out['clash_s'].shape)}")
    b = out["bonds"].reshape(-1, 2) if out["bonds"].size == 0 else out["bonds"]
    if b.ndim != 2 or b.shape[1] != 2:
        raise ValueError(f"bonds must have shape [B, 2], got {tuple(b.shape)}")
    b = b.astype(np.int64)
    bad = ((b < 0) | (b >= n_atoms)).any(axis=1) | (b[:, 0] == b[:, 1])
    if bad.any():
        j = int(np.flatnonzero(bad)[0])
        raise ValueError(f"bond {j}, {b[j].tolist()}, is not two different atoms in [0, {n_atoms})")
    B = int(b.shape[0])
    for key in ("bond_lo_s", "bond_hi_s"):
        if out[key].shape != (B,):
            raise ValueError(f"{key} must have shape [{B}], got {tuple(out[key].shape)}")
    out["bonds"] = b
    return {key: np.ascontiguousarray(out[key], dtype=dtype) for key, dtype in _VALIDITY_KEYS}


def upload_validity_tables(tables, n_atoms: int, device) -> Dict[str, torch.Tensor]:
    """`check_validity_tables`, then the four tables as tensors on ``device``: upload once, call `validity_counts` often."""
    return {key: torch.from_numpy(a).to(device) for key, a in check_validity_tables(tables, n_atoms).items()}


def validity_counts(frames: torch.Tensor, tables, out: Optional[torch.Tensor] = None, bond_frames=None):
    """Queue the chemical-validity counts of the frames ``frames [T, n, 3]`` (device fp32, a view of either trajectory layout, or any
    strided selection of its frames) on the current stream: ``(counts int32 [T, 2], bond_frames int32 [B])``, per frame the clashing
    non-bonded pairs and the bonds of a wrong length, per bond the frames in which it is off; `validity.validity_counts_host` is the
    specification and the counts equal it integer for integer.  ``tables``: the dict of `validity.validity_tables` (or its four arrays
    ``clash_s``, ``bonds``, ``bond_lo_s``, ``bond_hi_s``).  Host tables are checked (`check_validity_tables`) before anything needs a GPU
    and uploaded; tables whose ``bonds`` is a tensor on the device of ``frames`` (`upload_validity_tables`) are taken as checked: the
    kernel skips a bond with an index out of range, it never reads there.  ``out`` (contiguous int32 ``[T, 2]``) and ``bond_frames``
    (contiguous int32 ``[B]``) receive the result; default new tensors; ``bond_frames=False`` asks for none and returns ``None`` for it.
    The counters are unsigned 32-bit, handed out as int32 as `hist2d_pairs` hands out its own.  Nothing is read back.
    See ``jamun_validity_counts``."""
    if not torch.is_tensor(frames) or frames.ndim != 3 or frames.shape[2] != 3:
        raise RuntimeError(f"frames must be a [frames, atoms, 3] tensor, got {tuple(getattr(frames, 'shape', ()))}")
    n, T = int(frames.shape[1]), int(frames.shape[0])
    if not 1 <= n <= VALIDITY_MAX_ATOMS:
        raise ValueError(f"{n} atoms: the device path takes 1 to {VALIDITY_MAX_ATOMS} (validity.validity_counts_host has no limit)")
    on_device = _on_device(tables["bonds"])
    if not on_device:
        tables = check_validity_tables(tables, n)  # (before anything needs a GPU)
    fs, as_, _, _ = _frame_strides(frames)
    _fit_31_bits(f"{T} frames: the count must fit 31 bits", T)
    _lib.load()
    dev = frames.device
    B = int(tables["bonds"].shape[0])
    want = {"clash_s": (torch.float32, (n * (n - 1) // 2,)), "bonds": (torch.int32, (B, 2)), "bond_lo_s": (torch.float32, (B,)),
            "bond_hi_s": (torch.float32, (B,))}
    t = {key: _table(key, f"{dtype} {list(shape)}", tables[key], on_device, dev, dtype, shape) for key, (dtype, shape) in want.items()}
    out = _result("out", out, (T, 2), torch.int32, dev)
    # (zeros: with T == 0 the call writes nothing)
    bond_frames = None if bond_frames is False else _result("bond_frames", bond_frames, (B,), torch.int32, dev, fill=0)
    if T == 0 and bond_frames is not None:
        bond_frames.zero_()
    _call(dev, "jamun_validity_counts", _ptr(frames), fs, as_, n, T, _ptr(t["clash_s"]), _ptr(t["bonds"]), _ptr(t["bond_lo_s"]), _ptr(t["bond_hi_s"]), B,
          _ptr(out), int(out.numel()), _ptr(bond_frames))
    return out, bond_frames


# ---- lagged moments, projection and autocovariance sums of feature trajectories (jamun_tica.hip) -------------------------------------------

TICA_MAX_WIDTH = 128     # feature columns the moments and the projection take (JAMUN_TICA_MAX_WIDTH, jamun_internal.h)
TICA_MAX_ACF_LAG = 4096  # largest lag of the autocovariance sums (JAMUN_TICA_MAX_ACF_LAG)
TICA_SLICE = 1024        # frames whose terms one workgroup adds (JAMUN_TICA_SLICE)
TICA_TILE = 32           # rows and columns of the moment matrices a workgroup owns (JAMUN_TICA_TILE)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_feature_rows(x) -> Tuple[int, int]:
    """The shape rule of the feature rows `lagged_moments` and `project_frames` read, before anything needs a GPU: a ``[T, W]`` tensor
    with ``1 <= W <= 128`` (``ValueError`` otherwise).  Returns ``(T, W)``."""
    if not torch.is_tensor(x) or x.ndim != 2:
        raise ValueError(f"x must be a [frames, width] tensor, got {tuple(getattr(x, 'shape', ()))}")
    T, W = int(x.shape[0]), int(x.shape[1])
    if not 1 <= W <= TICA_MAX_WIDTH:
        raise ValueError(f"{W} feature columns: the device path takes 1 to {TICA_MAX_WIDTH} (tica.lagged_moments_host has no limit)")
    return T, W


def lagged_moments(x: torch.Tensor, lag: int, sums: Optional[torch.Tensor] = None,
                   moments: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Queue the lagged second moments of the feature rows ``x [T, W]`` (device fp32 with adjacent columns: what `internal_coords` returns
    with ``cossin``, or a view of it with a row stride) on the current stream: ``(sums float64 [2, W], moments float64 [3, W, W])`` over
    the ``T - lag`` pairs ``(x_t, x_{t+lag})``: the sums of ``x_t`` and of ``x_{t+lag}``, and ``G``, ``H``, ``K`` as
    `tica.lagged_moments_host` defines them.  ``1 <= lag < T`` and ``1 <= W <= 128`` (``ValueError`` otherwise, before anything needs a
    GPU).  ``sums`` / ``moments`` (contiguous float64 of those shapes on the device) receive the result; default new tensors.  The
    workspace is this module's.  Same inputs, same bits.  See ``jamun_lagged_moments``."""
    T, W = check_feature_rows(x)
    if not _is_int(lag) or not 1 <= int(lag) < T:
        raise ValueError(f"lag must be an integer in [1, {T}) for {T} frames, got {lag!r}")
    lag = int(lag)
    row_stride = _rows("x", x, torch.float32, "columns")
    _lib.load()
    dev = x.device
    sums = _result("sums", sums, (2, W), torch.float64, dev)
    moments = _result("moments", moments, (3, W, W), torch.float64, dev)
    _call(dev, "jamun_lagged_moments", _ptr(x), row_stride, T, W, lag, _ptr(sums), _ptr(moments), *_workspace_for(dev, "jamun_lagged_moments_work", T, W, lag))
    return sums, moments


def project_frames(x: torch.Tensor, mean, v, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the projection of the feature rows ``x [T, W]`` (as `lagged_moments` takes them) on the current stream: float64 ``[T, d]``,
    ``out[t] = (x[t] - mean) @ v`` with ``mean [W]`` and ``v [W, d]``, ``1 <= d <= W`` (float64; host arrays are uploaded, tensors on the
    device of ``x`` are used as they are).  ``out`` (contiguous float64 ``[T, d]`` on the device) receives the result; default a new
    tensor.  `tica.project_host` is the specification.  See ``jamun_project_frames``."""
    T, W = check_feature_rows(x)
    shape_v = tuple(getattr(v, "shape", ()))
    if tuple(getattr(mean, "shape", ())) != (W,) or len(shape_v) != 2 or shape_v[0] != W or not 1 <= shape_v[1] <= W:
        raise ValueError(f"mean must have shape [{W}] and v [{W}, d] with 1 <= d <= {W}, got {tuple(getattr(mean, 'shape', ()))} and {shape_v}")
    d = int(shape_v[1])
    row_stride = _rows("x", x, torch.float32, "columns")
    _lib.load()
    dev = x.device
    mean, v = _dense("mean", mean, torch.float64, dev), _dense("v", v, torch.float64, dev)
    out = _result("out", out, (T, d), torch.float64, dev)
    _call(dev, "jamun_project_frames", _ptr(x), row_stride, T, W, _ptr(mean), _ptr(v), d, _ptr(out), int(out.numel()))
    return out


def autocov_sums(y: torch.Tensor, max_lag: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the autocovariance sums of ``y [T]`` (device float64, any positive stride: a column of `project_frames`' result is read in
    place) on the current stream: float64 ``[max_lag + 1]``, ``out[k] = sum_{t < T - k} y[t] y[t + k]`` and 0 for ``k >= T``;
    ``0 <= max_lag <= 4096`` (``ValueError`` otherwise).  Dividing by ``T - k`` gives statsmodels' ``acovf(adjusted=True, demean=False)``.
    ``out`` (contiguous float64 of that shape on the device) receives the result; default a new tensor.  The workspace is this module's.
    Same inputs, same bits.  `tica.autocov_sums_host` is the specification.  See ``jamun_autocov_sums``."""
    if not torch.is_tensor(y) or y.ndim != 1:
        raise ValueError(f"y must be a [frames] tensor, got {tuple(getattr(y, 'shape', ()))}")
    if not _is_int(max_lag) or not 0 <= int(max_lag) <= TICA_MAX_ACF_LAG:
        raise ValueError(f"max_lag must be an integer in [0, {TICA_MAX_ACF_LAG}], got {max_lag!r}")
    max_lag, T = int(max_lag), int(y.shape[0])
    if not y.is_cuda or y.dtype != torch.float64 or (T > 1 and y.stride(0) < 1):
        raise RuntimeError(f"y must be a float64 tensor on the GPU with a positive stride, got {y.dtype} {tuple(y.shape)} strides {tuple(y.stride())} "
                           f"on {y.device}")
    _fit_31_bits(f"{T} frames: the count must fit 31 bits", T)
    _lib.load()
    dev = y.device
    out = _result("out", out, (max_lag + 1,), torch.float64, dev)
    work = _workspace_for(dev, "jamun_autocov_sums_work", T, max_lag)
    if T == 0:
        out.zero_()  # (no frame: the call writes nothing)
    _call(dev, "jamun_autocov_sums", _ptr(y), int(y.stride(0)) if T > 1 else 1, T, max_lag, _ptr(out), *work)
    return out


# ---- nearest centres, cluster sums, transition and occupancy counts (jamun_msm.hip) ----------------------------------------------------------

MSM_MAX_K = 1024         # centres `assign_centers` and `cluster_sums` take (JAMUN_MSM_MAX_K, jamun_internal.h)
MSM_MAX_D = 128          # columns of a row (JAMUN_MSM_MAX_D)
MSM_MAX_KD = 16384       # k * d at most (JAMUN_MSM_MAX_KD)
MSM_MAX_STATES = 1024    # states of the count tables (JAMUN_MSM_MAX_STATES)
MSM_MAX_SEGMENTS = 4096  # segments of `label_counts` (JAMUN_MSM_MAX_SEGMENTS)


def check_centers_shape(k: int, d: int) -> None:
    """The limits of the device path on ``k`` centres of ``d`` columns (``ValueError`` otherwise), before anything needs a GPU."""
    if not (1 <= k <= MSM_MAX_K and 1 <= d <= MSM_MAX_D and k * d <= MSM_MAX_KD):
        raise ValueError(f"k = {k} centres of d = {d} columns: the device path takes 1 <= k <= {MSM_MAX_K}, 1 <= d <= {MSM_MAX_D} and "
                         f"k * d <= {MSM_MAX_KD} (the host functions of jamun_amd.msm have no limit)")


def _projection_shape(y) -> Tuple[int, int]:
    """The shape rule of the rows `assign_centers` and `cluster_sums` read, before anything needs a GPU: ``[T, d]`` with ``1 <= d <= 128``."""
    if not torch.is_tensor(y) or y.ndim != 2:
        raise ValueError(f"y must be a [frames, d] tensor, got {tuple(getattr(y, 'shape', ()))}")
    T, d = int(y.shape[0]), int(y.shape[1])
    if not 1 <= d <= MSM_MAX_D:
        raise ValueError(f"{d} columns: the device path takes 1 to {MSM_MAX_D}")
    return T, d


def _labels(name: str, labels, device=None, T: Optional[int] = None) -> torch.Tensor:
    if (not torch.is_tensor(labels) or labels.ndim != 1 or labels.dtype != torch.int32 or not labels.is_cuda or not labels.is_contiguous()
            or (device is not None and labels.device != device) or (T is not None and int(labels.shape[0]) != T)):
        raise RuntimeError(f"{name} must be a contiguous int32 [{'frames' if T is None else T}] tensor on the GPU"
                           f"{'' if device is None else f' ({device})'}, got {getattr(labels, 'dtype', None)} {tuple(getattr(labels, 'shape', ()))} "
                           f"on {getattr(labels, 'device', None)}")
    _fit_31_bits(f"{labels.shape[0]} frames: the count must fit 31 bits", int(labels.shape[0]))
    return labels


def assign_centers(y: torch.Tensor, centers, labels: Optional[torch.Tensor] = None, sqdist=None, prev_labels: Optional[torch.Tensor] = None,
                   n_changed: Optional[torch.Tensor] = None):
    """Queue the nearest centre of every row of ``y [T, d]`` (device float64 with adjacent columns: what `project_frames` returns, or a
    view of it with a row stride) on the current stream.  ``centers [k, d]`` float64 (a host array is uploaded, a tensor on the device is
    used as it is).  Returns ``(labels int32 [T], sqdist float64 [T] or None, n_changed int64 [1] or None)``: the centre of smallest squared
    distance (the lowest index on a tie; -1 and a NaN distance for a row with a non-finite value), the distance to it where ``sqdist`` is
    ``True`` or a tensor to write to, and, with ``prev_labels`` (int32 ``[T]``), the number of labels that differ from it ADDED to
    ``n_changed`` (default a new zero).  Label and distance equal `msm.assign_centers_host` bit for bit.  See ``jamun_assign_centers``."""
    T, d = _projection_shape(y)
    shape_c = tuple(getattr(centers, "shape", ()))
    if len(shape_c) != 2 or shape_c[1] != d:
        raise ValueError(f"centers must have shape [k, {d}], got {shape_c}")
    k = int(shape_c[0])
    check_centers_shape(k, d)
    row_stride = _rows("y", y, torch.float64, "columns")
    dev = y.device
    centers = _dense("centers", centers, torch.float64, dev)
    if n_changed is not None and prev_labels is None:
        raise ValueError("n_changed needs prev_labels to compare with")
    _lib.load()
    labels = _result("labels", labels, (T,), torch.int32, dev)
    if sqdist is True:
        sqdist = torch.empty((T,), dtype=torch.float64, device=dev)
    elif sqdist is False:
        sqdist = None
    elif sqdist is not None:
        sqdist = _result("sqdist", sqdist, (T,), torch.float64, dev)
    if prev_labels is not None:
        prev_labels = _labels("prev_labels", prev_labels, dev, T)
        n_changed = _result("n_changed", n_changed, (1,), torch.int64, dev, fill=0)
    _call(dev, "jamun_assign_centers", _ptr(y), row_stride, T, d, _ptr(centers), k, _ptr(labels), _ptr(sqdist), _ptr(prev_labels), _ptr(n_changed))
    return labels, sqdist, n_changed


def cluster_sums(y: torch.Tensor, labels: torch.Tensor, k: int, counts: Optional[torch.Tensor] = None,
                 sums: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Queue the per-cluster sums of the rows ``y [T, d]`` (as `assign_centers` takes them; a ``[T]`` tensor counts as one column) on the
    current stream: ``(counts int64 [k], sums float64 [k, d])``, the rows carrying each label of ``labels`` (int32 ``[T]``; labels outside
    ``[0, k)`` are skipped) and their sum, added in the fixed order of `msm.cluster_sums_host`: the same bits as the host's, in every run.
    The workspace is this module's (shared with the TICA reductions).  See ``jamun_cluster_sums``."""
    if torch.is_tensor(y) and y.ndim == 1:
        y = y[:, None]
    T, d = _projection_shape(y)
    if not _is_int(k):
        raise ValueError(f"k must be an integer, got {k!r}")
    k = int(k)
    check_centers_shape(k, d)
    row_stride = _rows("y", y, torch.float64, "columns")
    dev = y.device
    labels = _labels("labels", labels, dev, T)
    _lib.load()
    counts = _result("counts", counts, (k,), torch.int64, dev)
    sums = _result("sums", sums, (k, d), torch.float64, dev)
    work = _workspace_for(dev, "jamun_cluster_sums_work", T, d, k)
    if T == 0:
        counts.zero_()  # (no frame: the call writes nothing)
        sums.zero_()
    _call(dev, "jamun_cluster_sums", _ptr(y), row_stride, T, d, _ptr(labels), k, _ptr(counts), _ptr(sums), *work)
    return counts, sums


def _state_map(state_map, n_states: int, dev) -> Tuple[Optional[torch.Tensor], int]:
    if not _is_int(n_states) or not 1 <= int(n_states) <= MSM_MAX_STATES:
        raise ValueError(f"n_states must be an integer in [1, {MSM_MAX_STATES}], got {n_states!r}")
    if state_map is None:
        return None, int(n_states)
    if not torch.is_tensor(state_map):
        state_map = _dense("state_map", state_map, torch.int32)  # (a host table is converted; a scalar becomes a table of one entry)
    if state_map.ndim != 1 or state_map.dtype != torch.int32 or state_map.shape[0] < 1:  # (its own text, so ahead of `_dense`'s)
        raise ValueError(f"state_map must be a non-empty int32 [n_in] table, got {state_map.dtype} {tuple(state_map.shape)}")
    _fit_31_bits("state_map: the length must fit 31 bits", int(state_map.shape[0]))
    return _dense("state_map", state_map, torch.int32, dev), int(state_map.shape[0])


def transition_counts(labels: torch.Tensor, lag: int, n_states: int, state_map=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the sliding transition counts of ``labels`` (device int32 ``[T]``) at ``lag >= 1`` on the current stream: int64
    ``[n_states, n_states]``, ``out[a, b]`` INCREASED by the number of ``t < T - lag`` with ``state(t) = a`` and ``state(t + lag) = b``.
    ``state_map`` (int32 ``[n_in]``, -1 for none; host array or device tensor) takes a label to its state; without it the label is the
    state.  Pairs with a label or state out of range are skipped.  ``out`` (contiguous int64 of that shape on the device) is added to: hand
    the same tensor in for every chain; default a new zero tensor.  `msm.transition_counts_host` is the specification."""
    labels = _labels("labels", labels)
    dev = labels.device
    if not _is_int(lag) or int(lag) < 1:
        raise ValueError(f"lag must be an integer of at least 1, got {lag!r}")
    _fit_31_bits("lag must fit 31 bits", int(lag))
    state_map, n_in = _state_map(state_map, n_states, dev)
    n_states = int(n_states)
    _lib.load()
    out = _result("out", out, (n_states, n_states), torch.int64, dev, fill=0)
    _call(dev, "jamun_transition_counts", _ptr(labels), int(labels.shape[0]), int(lag), _ptr(state_map), n_in, n_states, _ptr(out))
    return out


def label_counts(labels: torch.Tensor, bounds, n_states: int, state_map=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the occupancy counts of ``labels`` (device int32 ``[T]``) over the segments ``bounds[s] <= t < bounds[s + 1]`` on the current
    stream: int64 ``[n_seg, n_states]``, INCREASED by the frames of every segment in every state.  ``bounds`` int32 ``[n_seg + 1]``,
    non-decreasing within ``[0, T]`` (a host array is checked and uploaded; a device tensor is taken as checked), ``state_map`` and
    ``out`` as in `transition_counts`.  `msm.label_counts_host` is the specification."""
    labels = _labels("labels", labels)
    dev, T = labels.device, int(labels.shape[0])
    state_map, n_in = _state_map(state_map, n_states, dev)
    n_states = int(n_states)
    if not _on_device(bounds):
        b = np.asarray(bounds)
        if b.ndim != 1 or b.shape[0] < 2 or not np.issubdtype(b.dtype, np.integer) or (np.diff(b) < 0).any() or b[0] < 0 or b[-1] > T:
            raise ValueError(f"bounds must be at least two non-decreasing integers within [0, {T}], got {b.tolist() if b.size <= 16 else b.shape}")
        bounds = np.ascontiguousarray(b, dtype=np.int32)
    bounds = _table("bounds", "int32 [n_seg + 1]", bounds, _on_device(bounds), dev, torch.int32, (None,))
    n_seg = int(bounds.shape[0]) - 1
    if not 1 <= n_seg <= MSM_MAX_SEGMENTS:
        raise ValueError(f"{n_seg} segments: the device path takes 1 to {MSM_MAX_SEGMENTS}")
    _lib.load()
    out = _result("out", out, (n_seg, n_states), torch.int64, dev, fill=0)
    _call(dev, "jamun_label_counts", _ptr(labels), T, _ptr(state_map), n_in, n_states, _ptr(bounds), n_seg, _ptr(out))
    return out


# ---- sliced Wasserstein distance: projection, segment sort, merge, quantile integral (jamun_swd.hip) ---------------------------------------

SWD_TILE = 4096      # keys a workgroup sorts in LDS, the unit of the merge passes (JAMUN_SWD_TILE, jamun_internal.h)
SWD_MAX_WIDTH = 128  # descriptor columns `swd_project` takes (JAMUN_SWD_MAX_WIDTH)
SWD_MAX_PROJ = 64    # directions (JAMUN_SWD_MAX_PROJ)


def check_swd_shapes(width: int, n_proj: int) -> None:
    """The limits of the device path on the descriptor columns and the directions (``ValueError`` otherwise), before anything needs a GPU."""
    if not (1 <= width <= SWD_MAX_WIDTH and 1 <= n_proj <= SWD_MAX_PROJ):
        raise ValueError(f"{width} descriptor columns on {n_proj} directions: the device path takes 1 to {SWD_MAX_WIDTH} columns and 1 to "
                         f"{SWD_MAX_PROJ} directions (the host functions of jamun_amd.swd have no limit)")


def _swd_columns(name: str, a) -> Tuple[int, int]:
    """The shape rule of a set of key columns ``[L, n]``, before anything needs a GPU: ``1 <= L <= 64``, ``n >= 1``.  Returns ``(L, n)``."""
    if not torch.is_tensor(a) or a.ndim != 2 or a.shape[1] < 1 or not 1 <= a.shape[0] <= SWD_MAX_PROJ:
        raise ValueError(f"{name} must be a [directions, keys] tensor of 1 to {SWD_MAX_PROJ} directions and at least one key, got "
                         f"{tuple(getattr(a, 'shape', ()))}")
    return int(a.shape[0]), int(a.shape[1])


def swd_project(x: torch.Tensor, proj, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the projection of the descriptor rows ``x [T, W]`` (device fp32 with adjacent columns: what `internal_coords` returns with
    ``cossin``, or a view of it with a row stride) on the directions ``proj [W, L]`` (float32; a host array is uploaded, a tensor on the
    device is used as it is) on the current stream: float32 ``[L, T]``, bit for bit `swd.project_host`.  ``T >= 1``, ``1 <= W <= 128``,
    ``1 <= L <= 64`` (``ValueError`` otherwise, before anything needs a GPU).  ``out`` (contiguous float32 of that shape on the device)
    receives the result; default a new tensor.  See ``jamun_swd_project``."""
    if not torch.is_tensor(x) or x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f"x must be a [frames, width] tensor of at least one frame, got {tuple(getattr(x, 'shape', ()))}")
    T, W = int(x.shape[0]), int(x.shape[1])
    shape_p = tuple(getattr(proj, "shape", ()))
    if len(shape_p) != 2 or shape_p[0] != W:
        raise ValueError(f"proj must have shape [{W}, L], got {shape_p}")
    L = int(shape_p[1])
    check_swd_shapes(W, L)
    proj = _dense("proj", proj, torch.float32, convert=False)  # (a host array of another type is refused, not converted; uploaded below)
    row_stride = _rows("x", x, torch.float32, "columns")
    _lib.load()
    dev = x.device
    proj = proj.to(dev)
    out = _result("out", out, (L, T), torch.float32, dev)
    _call(dev, "jamun_swd_project", _ptr(x), row_stride, T, W, _ptr(proj), L, _ptr(out), int(out.numel()))
    return out


def swd_sort_segments(keys: torch.Tensor, cuts, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the sort of every segment of every column of ``keys [L, T]`` (contiguous device fp32: what `swd_project` returns) on the
    current stream: float32 ``[L, T]`` whose frames ``cuts[c-1] <= t < cuts[c]`` are sorted by `swd.order_image`, each segment on its
    own; frames from the last cut on are copied.  ``cuts`` as `check_cuts` takes them (a host array).  Out of place; ``out`` (contiguous
    float32 of that shape on the device) receives the result and may be ``keys`` itself; default a new tensor.  The workspace of the merge
    passes is this module's.  `swd.sort_segments_host` is the specification: the bits are its bits.  See ``jamun_swd_sort_segments``."""
    L, T = _swd_columns("keys", keys)
    cuts = np.ascontiguousarray(check_cuts(cuts, T), dtype=np.int32)
    if _rows("keys", keys, torch.float32, "keys") != T:
        raise RuntimeError(f"keys must be contiguous, got strides {tuple(keys.stride())}")
    _lib.load()
    dev = keys.device
    out = _result("out", out, (L, T), torch.float32, dev)
    cut_args = (cuts.ctypes.data, int(cuts.shape[0]))
    _call(dev, "jamun_swd_sort_segments", _ptr(keys), T, L, *cut_args, _ptr(out), int(out.numel()),
          *_workspace_for(dev, "jamun_swd_sort_work", T, L, *cut_args, dtype=torch.float32))
    return out


def swd_merge(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the merge of the sorted columns ``a [L, n]`` and ``b [L, m]`` (device fp32 with adjacent keys; a row stride is taken, so a
    segment of `swd_sort_segments`' result is read in place) on the current stream: float32 ``[L, n + m]``, sorted by `swd.order_image`.
    ``out`` (contiguous float32 of that shape on the device, apart from both) receives the result; default a new tensor.
    `swd.merge_sorted_host` is the specification.  See ``jamun_swd_merge``."""
    L, n = _swd_columns("a", a)
    Lb, m = _swd_columns("b", b)
    if Lb != L:
        raise ValueError(f"a and b must have the same number of directions, got {L} and {Lb}")
    if n + m > 0x7FFFFFFF:
        raise ValueError(f"{n} + {m} keys: the sum must fit 31 bits")
    sa = _rows("a", a, torch.float32, "keys")
    sb = _rows("b", b, torch.float32, "keys", a.device)
    _lib.load()
    out = _result("out", out, (L, n + m), torch.float32, a.device)
    _call(a.device, "jamun_swd_merge", _ptr(a), sa, n, _ptr(b), sb, m, L, _ptr(out), int(out.numel()))
    return out


def swd_w2sq(u: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Queue the squared 2-Wasserstein distances of the sorted columns ``u [L, n]`` and ``v [L, m]`` (as `swd_merge` takes them) on the
    current stream: float64 ``[L]``, the quantile integral of `swd.w2sq_sorted_host` with every term formed as there and added in a
    fixed order: the same bits in every run, within ``(n + m) 2^-52`` relative of the specification.  ``out`` (contiguous float64 ``[L]`` on
    the device) receives the result; default a new tensor.  The workspace is this module's.  See ``jamun_swd_w2sq``."""
    L, n = _swd_columns("u", u)
    Lv, m = _swd_columns("v", v)
    if Lv != L:
        raise ValueError(f"u and v must have the same number of directions, got {L} and {Lv}")
    su = _rows("u", u, torch.float32, "keys")
    sv = _rows("v", v, torch.float32, "keys", u.device)
    _lib.load()
    dev = u.device
    out = _result("out", out, (L,), torch.float64, dev)
    _call(dev, "jamun_swd_w2sq", _ptr(u), su, n, _ptr(v), sv, m, L, _ptr(out), *_workspace_for(dev, "jamun_swd_w2sq_work", n, m, L))
    return out
