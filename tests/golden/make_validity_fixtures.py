"""Records what the REFERENCE'S OWN functions count on this repository's chemical-validity cases -> tests/golden/validity_reference.npz.

    python tests/golden/make_validity_fixtures.py        # needs the reference checkout (JAMUN_REFERENCE_SRC, default /root/reference/src)

The reference's ``metrics/_chemical_validity.py`` is loaded from its file.  Its imports at module level (mdtraj, wandb, lightning, its own
package) are not installed here and are not needed: the two functions recorded, ``_check_volume_exclusion`` and ``_check_bond_lengths``,
use numpy only, so empty stand-ins are put into ``sys.modules`` before the file is executed.  No reference source is copied; only the
recorded integers are committed.

Cases (inputs from tests/_validity_cases.py, regenerated from their seeds by the test; the reference is given the bonds lower index first,
as mdtraj hands them over):
    dipeptide_ref    the Ala-Gly dipeptide, 200 noisy frames, the reference's tolerances (0.1, 0.2)
    dipeptide_wide   the same frames at (0.35, 0.2), where the structure itself is clean
    sulphur          the dipeptide with its CB replaced by S at (0.1, 0.2): the reference's covalent radius of sulphur, 1.005
    helix10          ten atoms of the helix (C, N, O), 129 noisy frames, (0.3, 0.2)
Per case: ``<case>_counts`` int64 [T, 2] (issues of either kind per frame) and ``<case>_bond_frames`` int64 [B] (frames in which the bond,
in sorted order, is an issue).

The script asserts that no input distance lies within 4 float32 ulp of a threshold it is compared with: there the outcome of the
reference's ``float32 < float`` depends on numpy's scalar promotion rule (numpy 1 promotes to float64, numpy 2 compares in float32), so
such an input would pin a numpy version, not the metric.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SRC = os.environ.get("JAMUN_REFERENCE_SRC", "/root/reference/src")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import _validity_cases as vc  # noqa: E402
from _traj_molecules import dipeptide  # noqa: E402

OUT = os.path.join(HERE, "validity_reference.npz")


def cases() -> dict:
    """name -> (molecule, (vtol, btol), frames float32 [T, n, 3])."""
    sulphur = dict(dipeptide())
    sulphur["elements"] = [e if i != 2 else "S" for i, e in enumerate(sulphur["elements"])]
    return {"dipeptide_ref": (dipeptide(), vc.REFERENCE_TOLERANCES, vc.dipeptide_frames(200)),
            "dipeptide_wide": (dipeptide(), vc.DIPEPTIDE_TOLERANCES, vc.dipeptide_frames(200)),
            "sulphur": (sulphur, vc.REFERENCE_TOLERANCES, vc.dipeptide_frames(200)),
            "helix10": (vc.helix(10), vc.HELIX_TOLERANCES, vc.helix_frames(10, 129))}


def sorted_bonds(mol: dict) -> list:
    return sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in np.asarray(mol["bonds"]).T.tolist()})


def load_reference():
    class _Anything(types.ModuleType):
        def __getattr__(self, name):  # whatever the file names at import time: a class to derive from, a decorator's owner
            if name.startswith("__"):
                raise AttributeError(name)
            return type(name, (), {})

    for name in ("mdtraj", "wandb", "lightning", "lightning.pytorch", "lightning.pytorch.utilities", "jamun", "jamun.utils", "jamun.metrics",
                 "jamun.metrics._utils"):
        sys.modules.setdefault(name, _Anything(name))
    path = os.path.join(REF_SRC, "jamun", "metrics", "_chemical_validity.py")
    spec = importlib.util.spec_from_file_location("_reference_chemical_validity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assert_clear_of_thresholds(ref, mol, tol, frames) -> float:
    """The least distance, in float32 ulp, between an input distance and a threshold it is compared with; asserts it is above 4."""
    vtol, btol = tol
    el, bonded = list(mol["elements"]), set(sorted_bonds(mol))
    x = np.asarray(frames, dtype=np.float64)
    least = np.inf
    for i in range(x.shape[1]):
        for j in range(i + 1, x.shape[1]):
            d = np.linalg.norm(np.asarray(frames)[:, i] - np.asarray(frames)[:, j], axis=1).astype(np.float64)
            if (i, j) in bonded:
                c = ref.COVALENT_RADII[el[i]] + ref.COVALENT_RADII[el[j]]
                thrs = [(1 + btol) * c, (1 - btol) * c]
            else:
                thrs = [(1 - vtol) * (ref.VDW_RADII[el[i]] + ref.VDW_RADII[el[j]])]
            for thr in thrs:
                least = min(least, float(np.abs(d - thr).min() / np.spacing(np.float32(thr))))
    assert least > 4.0, f"an input distance lies {least:.2f} float32 ulp from a threshold: take another seed"
    return least


def main() -> None:
    ref = load_reference()
    out = {"numpy_version": np.array(np.__version__)}
    for name, (mol, tol, frames) in cases().items():
        least = assert_clear_of_thresholds(ref, mol, tol, frames)
        bonds = sorted_bonds(mol)
        el = np.array(list(mol["elements"]))
        clashes = ref._check_volume_exclusion(np.array(frames), el, bonds, tol[0])
        off = ref._check_bond_lengths(np.array(frames), el, bonds, tol[1])
        counts = np.array([[len(a), len(b)] for a, b in zip(clashes, off)], dtype=np.int64)
        bond_frames = np.array([sum((b in frame) for frame in off) for b in bonds], dtype=np.int64)
        assert not any(p in set(bonds) for frame in clashes for p in frame) and all(p in set(bonds) for frame in off for p in frame)
        out[f"{name}_counts"], out[f"{name}_bond_frames"] = counts, bond_frames
        print(f"{name}: {counts.shape[0]} frames, mean issues {counts.mean(axis=0).round(3).tolist()}, nearest threshold {least:.1f} ulp away")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
