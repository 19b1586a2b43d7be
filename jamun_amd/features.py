"""Internal coordinates of trajectory frames: which atoms (backbone and side-chain torsions, C-alpha pairs), and their values.

What every consumer of the reference's trajectories starts from (``md.compute_phi`` / ``md.compute_psi`` in
``metrics/_ramachandran.py``; backbone and side-chain torsions, plain and as cos / sin pairs, and C-alpha distances in
``analysis/utils.py``).  A feature is a row of an index table ``[F, 4]``: 2, 3 or 4 atom indices followed by ``-1``:

    2  distance    |p1 - p0|  (nm)
    3  bond angle at p1    atan2(|a x b|, a.b)  with a = p0 - p1, b = p2 - p1, in [0, pi]   (never acos: it loses half the digits near 0 and pi)
    4  dihedral    b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2:  atan2((b1.c1) |b2|, c1.c2) in (-pi, pi]
                   (mdtraj's form, the IUPAC sign)

The result is ``[T, F]``; with ``cossin`` it is ``[T, 2 F]``, interleaved ``(cos, sin)`` pairs of the angles and dihedrals taken from the two
atan2 arguments themselves (``(x, y) / |(x, y)|``: continuous across +-pi), a distance as ``(d, 0)``.  A row with fewer than two leading
indices or with an index outside ``[0, n)`` is NaN; so is a feature of which an atom has a non-finite coordinate in that frame, and nothing
else.  Where both atan2 arguments vanish (coincident atoms, a collinear triple inside a dihedral) the value is atan2's, 0 or pi, with
``(cos, sin) = (+-1, 0)``.

`internal_coords_host` is the specification (numpy, float64) and the host path; ``native.internal_coords`` (``jamun_intcoord.hip``: one
lane per frame, fp32) is the device path.  `internal_coords` picks between them.  `torsion_indices` and `ca_distance_indices` build the
tables from a molecule dict (`pdb.read_pdb`) by atom names, residue by residue: mdtraj's rule.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch


def _as_numpy(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _cross(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (a * b).sum(axis=-1)


def _angle_or_pair(y: np.ndarray, x: np.ndarray, cossin: bool) -> Tuple[np.ndarray, np.ndarray]:
    """atan2(y, x), or (cos, sin) of it from (x, y) normalised; x = y = 0 gives atan2's 0 or pi and (+-1, 0)."""
    if not cossin:
        return np.arctan2(y, x), np.zeros_like(x)
    m = np.maximum(np.abs(x), np.abs(y))
    zero = m == 0
    ms = np.where(zero, 1.0, m)
    xs, ys = x / ms, y / ms
    r = np.sqrt(xs * xs + ys * ys)
    r = np.where(zero, 1.0, r)
    return np.where(zero, np.copysign(1.0, x), xs / r), np.where(zero, 0.0, ys / r)


def internal_coords_host(frames, index, cossin: bool = False) -> np.ndarray:
    """``frames [T, n, 3]`` (any float type, tensor or array; nm) and ``index [F, 4]`` (integers) -> float64 ``[T, F]``, or ``[T, 2 F]``
    with ``cossin``.  The specification of ``jamun_internal_coords``; rows it would reject (`native.check_index_table`) give NaN here."""
    x = np.asarray(_as_numpy(frames), dtype=np.float64)
    idx = np.asarray(_as_numpy(index))
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"expected frames [T, n, 3], got {x.shape}")
    if idx.size == 0:
        idx = idx.reshape(-1, 4).astype(np.int64)
    if idx.dtype.kind not in "iu" or idx.ndim != 2 or idx.shape[1] != 4:
        raise ValueError(f"the index table must be an integer [F, 4] array, got {idx.dtype} {idx.shape}")
    T, n, F = x.shape[0], x.shape[1], idx.shape[0]
    mult = 2 if cossin else 1
    out = np.full((T, F * mult), np.nan)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(F):
            row = [int(v) for v in idx[j]]
            k = next((i for i, v in enumerate(row) if v < 0), 4)
            if k < 2 or any(v >= n for v in row[:k]):
                continue
            p = [x[:, v, :] for v in row[:k]]
            ok = np.isfinite(np.stack(p, axis=1)).all(axis=(1, 2))
            if k == 2:
                d = p[1] - p[0]
                v0, v1 = np.sqrt(_dot(d, d)), np.zeros(T)
            elif k == 3:
                a, b = p[0] - p[1], p[2] - p[1]
                c = _cross(a, b)
                v0, v1 = _angle_or_pair(np.sqrt(_dot(c, c)), _dot(a, b), cossin)
            else:
                b1, b2, b3 = p[1] - p[0], p[2] - p[1], p[3] - p[2]
                c1, c2 = _cross(b2, b3), _cross(b1, b2)
                v0, v1 = _angle_or_pair(_dot(b1, c1) * np.sqrt(_dot(b2, b2)), _dot(c1, c2), cossin)
            if cossin:
                out[:, 2 * j] = np.where(ok, v0, np.nan)
                out[:, 2 * j + 1] = np.where(ok, v1, np.nan)
            else:
                out[:, j] = np.where(ok, v0, np.nan)
    return out


def internal_coords(frames, index, cossin: bool = False):
    """The public call: ``[T, F]`` (``[T, 2 F]`` with ``cossin``) internal coordinates of ``frames [T, n, 3]``.  Float32 tensors on a GPU go
    to the HIP kernel (float32 out, no copy of a strided chain view) when the native library loads; everything else goes through
    `internal_coords_host` (float64 out).  Tensors in, tensors out (on the device of ``frames``); arrays in, arrays out."""
    if torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.float32:
        from . import _lib, native

        if _lib.available():
            return native.internal_coords(frames, index, cossin=cossin)
    out = internal_coords_host(frames, index, cossin=cossin)
    return torch.from_numpy(out).to(frames.device) if torch.is_tensor(frames) else out


# ---- which atoms -------------------------------------------------------------------------------------------------------------------------

# (the three fixed atoms, the alternatives for the fourth), the first pattern whose atoms all exist in the residue: mdtraj's CHI*_ATOMS
_CHI = {
    "CHI1": [(("N", "CA", "CB"), ("CG", "CG1", "SG", "OG", "OG1"))],
    "CHI2": [(("CA", "CB", "CG"), ("CD", "CD1", "OD1", "ND1", "SD")), (("CA", "CB", "CG1"), ("CD1",))],
    "CHI3": [(("CB", "CG", "CD"), ("NE", "CE", "OE1")), (("CB", "CG", "SD"), ("CE",))],
    "CHI4": [(("CG", "CD", "NE"), ("CZ",)), (("CG", "CD", "CE"), ("NZ",))],
}


def _residues(mol: dict) -> List[dict]:
    """The residues of ``mol`` in file order: ``{"name", "seq", "chain", "atoms": name -> atom index}``.  A residue is a run of atoms with one
    ``residue_sequence_index`` (and one chain); of two atoms of a name in a residue the first counts."""
    if mol is None or mol.get("atom_names") is None:
        raise ValueError("the molecule has no atom names (atom_names): torsions are found by name")
    names = list(mol["atom_names"])
    n = len(names)
    seq = [int(i) for i in mol["residue_sequence_index"]] if mol.get("residue_sequence_index") is not None else [0] * n
    resn = list(mol["residues"]) if mol.get("residues") is not None else ["UNK"] * n
    chain = [int(c) for c in mol["chain_index"]] if mol.get("chain_index") is not None else [0] * n
    if not (len(seq) == len(resn) == len(chain) == n):
        raise ValueError("atom_names, residues, residue_sequence_index and chain_index differ in length")
    out: List[dict] = []
    for i in range(n):
        if not out or out[-1]["seq"] != seq[i] or out[-1]["chain"] != chain[i]:
            out.append({"name": resn[i], "seq": seq[i], "chain": chain[i], "atoms": {}})
        out[-1]["atoms"].setdefault(names[i], i)
    return out


def torsion_indices(mol: dict, backbone: bool = True, sidechain: bool = False) -> Tuple[np.ndarray, List[str]]:
    """``(index int32 [F, 4], labels)`` of the torsions of ``mol`` (a molecule dict with ``atom_names``, ``residues``,
    ``residue_sequence_index``, as `pdb.read_pdb` returns it), by atom names only, neighbours being consecutive residues of one chain:
    phi of residue i = C(i-1) N CA C, psi = N CA C N(i+1), omega = CA C N(i+1) CA(i+1), chi1..chi4 by the first matching pattern of
    mdtraj's tables; each only where all four atoms exist.  Order: all phi in residue order, then psi, omega, chi1, chi2, chi3, chi4.
    Labels: ``"PHI 0 ALA 2"`` = kind, running number within the kind, residue name, residue sequence index."""
    res = _residues(mol)
    found: Dict[str, list] = {k: [] for k in ("PHI", "PSI", "OMEGA", "CHI1", "CHI2", "CHI3", "CHI4")}
    for r, cur in enumerate(res):
        prev = res[r - 1] if r > 0 and res[r - 1]["chain"] == cur["chain"] else None
        nxt = res[r + 1] if r + 1 < len(res) and res[r + 1]["chain"] == cur["chain"] else None
        a = cur["atoms"]
        if backbone:
            quads = {"PHI": (prev and prev["atoms"].get("C"), a.get("N"), a.get("CA"), a.get("C")),
                     "PSI": (a.get("N"), a.get("CA"), a.get("C"), nxt and nxt["atoms"].get("N")),
                     "OMEGA": (a.get("CA"), a.get("C"), nxt and nxt["atoms"].get("N"), nxt and nxt["atoms"].get("CA"))}
            for kind, quad in quads.items():
                if all(q is not None for q in quad):
                    found[kind].append((quad, cur))
        if sidechain:
            for kind, patterns in _CHI.items():
                for fixed, last in patterns:
                    if all(f in a for f in fixed) and any(l in a for l in last):
                        found[kind].append((tuple(a[f] for f in fixed) + (a[next(l for l in last if l in a)],), cur))
                        break
    rows, labels = [], []
    for kind, items in found.items():
        for number, (quad, cur) in enumerate(items):
            rows.append(quad)
            labels.append(f"{kind} {number} {cur['name']} {cur['seq']}")
    return np.array(rows, dtype=np.int32).reshape(-1, 4), labels


def ca_distance_indices(mol: dict, min_separation: int = 1) -> Tuple[np.ndarray, List[str]]:
    """``(index int32 [F, 4], labels)`` of the distances between the ``CA`` atoms of residues at least ``min_separation`` residues apart
    (counted over the residues that have a CA, in file order): rows ``[i, j, -1, -1]``, labels ``"CA-CA ALA 0 GLY 1"``."""
    if min_separation < 1:
        raise ValueError(f"min_separation must be at least 1, got {min_separation}")
    cas = [r for r in _residues(mol) if "CA" in r["atoms"]]
    rows, labels = [], []
    for i in range(len(cas)):
        for j in range(i + min_separation, len(cas)):
            rows.append((cas[i]["atoms"]["CA"], cas[j]["atoms"]["CA"], -1, -1))
            labels.append(f"CA-CA {cas[i]['name']} {cas[i]['seq']} {cas[j]['name']} {cas[j]['seq']}")
    return np.array(rows, dtype=np.int32).reshape(-1, 4), labels
