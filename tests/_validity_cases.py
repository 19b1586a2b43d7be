"""Cases for the chemical-validity tests (test_validity_host.py, test_gpu_validity.py, golden/make_validity_fixtures.py): seeded, no GPU.

MOLECULES.  The Ala-Gly dipeptide of the trajectory tests and `synth.random_chain` with names (`_traj_molecules`), and `helix(n, bonds)`:
n atoms on a helix of radius 0.2 nm, 40 degrees and 0.06 nm per atom, so that neighbours are 0.150 nm apart and every other pair at least
0.28 nm; elements cycle through C, N, O with an element no table knows ("Xx") every 11th atom.  Its bonds are chosen: "none", "tree" (the
chain k - (k + 1)) or "all" (every pair: nothing is left to clash, and every bond but the chain's is off in every frame).  With
HELIX_TOLERANCES = (0.3, 0.2) and the default radii the helix itself has no issue of either kind: the largest clash threshold,
0.7 * 0.34 = 0.238 nm, is below 0.28, and 0.150 lies inside (1 +- 0.2) times every sum of two covalent radii of C, N, O and "other"
(0.110 .. 0.182).

FRAMES.  `noisy_frames(pos, T)`: the structure plus Gaussian noise whose level cycles through NOISE (0.04, 0, 0.015, 0.004 nm) from frame
to frame, every frame shifted by up to 0.5 nm: a frame without noise has the structure's own counts (zero where the structure is clean),
0.04 nm moves a pair distance by 0.057 nm (one sigma), far past the 0.04 between the helix's 1-3 distance and its clash threshold and the
0.03 between its bonds and their limits.  `check_varied` asserts on the HOST counts that each count is zero in some frames and non-zero in
others, so that no test compares all-zero arrays.

DIPEPTIDE_TOLERANCES = (0.35, 0.2): the extended dipeptide's 1-3 pairs (0.24 nm) lie under the reference's clash threshold at its default
tolerance 0.1 (0.29 nm), as they do in every real molecule; at 0.35 the structure is clean and the noise decides.  REFERENCE_TOLERANCES =
(0.1, 0.2) are the reference's own.
"""
import functools

import numpy as np
import torch

from _traj_molecules import dipeptide

NOISE = (0.04, 0.0, 0.015, 0.004)  # nm, frame t gets NOISE[t % 4]
HELIX_TOLERANCES = (0.3, 0.2)
DIPEPTIDE_TOLERANCES = (0.35, 0.2)
REFERENCE_TOLERANCES = (0.1, 0.2)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)  # (cached and shared among the tests: read only)
    return a


def helix_bonds(n: int, kind: str) -> np.ndarray:
    """int64 [2, B], stored as a topology may store them: some higher index first, one bond twice."""
    if kind == "none" or n < 2:
        return np.zeros((2, 0), dtype=np.int64)
    if kind == "tree":
        rows = [(k - 1, k) for k in range(1, n)]
        rows = [(b, a) if k % 3 == 0 else (a, b) for k, (a, b) in enumerate(rows)] + [rows[0]]
    elif kind == "all":
        rows = [(i, j) for i in range(n) for j in range(i + 1, n)]
    else:
        raise KeyError(kind)
    return np.array(rows, dtype=np.int64).T.reshape(2, -1)


@functools.lru_cache(maxsize=None)
def helix(n: int, kind: str = "tree") -> dict:
    k = np.arange(n)
    th = np.deg2rad(40.0) * k
    pos = np.stack([0.2 * np.cos(th), 0.2 * np.sin(th), 0.06 * k], axis=1)
    elements = ["Xx" if i % 11 == 10 else ["C", "N", "O"][i % 3] for i in range(n)]
    return dict(pos=torch.tensor(pos - pos.mean(axis=0), dtype=torch.float32), elements=elements, bonds=torch.from_numpy(helix_bonds(n, kind)),
                atom_type_index=torch.tensor([{"C": 0, "O": 1, "N": 2}.get(e, 5) for e in elements], dtype=torch.int32),
                atom_names=[f"{e[0]}{i % 100}" for i, e in enumerate(elements)])


def noisy_frames(pos, T: int, seed: int = 0) -> np.ndarray:
    """float32 [T, n, 3]: see the module docstring."""
    rng = np.random.RandomState(seed)
    pos = np.asarray(pos, dtype=np.float64)
    shift = rng.randn(T, 1, 3)
    shift *= rng.uniform(0.0, 0.5, size=(T, 1, 1)) / np.linalg.norm(shift, axis=2, keepdims=True)
    sigma = np.array([NOISE[t % len(NOISE)] for t in range(T)])[:, None, None]
    return _frozen((pos[None] + shift + sigma * rng.randn(T, pos.shape[0], 3)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def helix_frames(n: int, T: int) -> np.ndarray:
    return noisy_frames(helix(n)["pos"].numpy(), T, seed=1000 + n)


@functools.lru_cache(maxsize=None)
def dipeptide_frames(T: int = 200) -> np.ndarray:
    return noisy_frames(dipeptide()["pos"].numpy(), T, seed=7)


def check_varied(counts: np.ndarray, which=(0, 1)) -> None:
    """Each count (0 clashes, 1 bad bonds) is zero in some frames and non-zero in others."""
    for k in which:
        col = np.asarray(counts)[:, k]
        assert (col == 0).any() and (col > 0).any(), (k, col[:16].tolist())


def plain_loop(frames: np.ndarray, mol: dict, vtol: float, btol: float, vdw: dict, cov: dict):
    """An independent check, written for the tests: per frame and pair sqrt in float32 and the comparison with the float64 threshold, as
    the reference compares them; returns ``(counts int64 [T, 2], bond_frames int64 [B], bonds)``."""
    x = np.asarray(frames, dtype=np.float32)
    T, n = x.shape[0], x.shape[1]
    el = list(mol["elements"])
    bonds = sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in np.asarray(mol["bonds"]).T.tolist()})
    bonded = set(bonds)
    r = lambda table, e: table[e] if e in table else table["other"]
    counts = np.zeros((T, 2), dtype=np.int64)
    bond_frames = np.zeros(len(bonds), dtype=np.int64)
    for t in range(T):
        for i in range(n):
            for j in range(i + 1, n):
                d = x[t, j] - x[t, i]
                dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                assert dist.dtype == np.float32
                if (i, j) in bonded:
                    c = r(cov, el[i]) + r(cov, el[j])
                    if float(dist) > (1 + btol) * c or float(dist) < (1 - btol) * c:
                        counts[t, 1] += 1
                        bond_frames[bonds.index((i, j))] += 1
                elif float(dist) < (1 - vtol) * (r(vdw, el[i]) + r(vdw, el[j])):
                    counts[t, 0] += 1
    return counts, bond_frames, bonds


def chain_batches(mol: dict, device, chains: int, T: int, n_batches: int, seed: int):
    """Samples as `unbatch_samples` hands them out ([n, T, 3] views of one [T, sum N, 3] tensor on ``device``): `noisy_frames` of the
    molecule, another seed for every chain."""
    pos = mol["pos"].numpy()
    n = pos.shape[0]
    out = []
    for b in range(n_batches):
        traj = np.concatenate([noisy_frames(pos, T, seed=seed + 10 * b + c) for c in range(chains)], axis=1)
        traj = torch.from_numpy(traj).to(device)
        out.append([{"dataset_label": "m", "atom_type_index": mol["atom_type_index"], "xhat_traj": traj[:, c * n : (c + 1) * n].permute(1, 0, 2)}
                    for c in range(chains)])
    return out
