"""Cases for the internal-coordinate tests (test_intcoord_host.py, test_gpu_intcoord.py): seeded, no GPU.

ANALYTIC cases are the oracle: geometry built FROM the answer, so the expected value is the number the case was made of, neither the
kernel's nor a library's.
  dihedral  p1 = 0, p2 = r2 z, p0 = r1 (sin b1, 0, cos b1) (in the xz-plane, x > 0), p3 = p2 + r3 (sin b2 cos th, sin b2 sin th, -cos b2):
            mdtraj's formula gives exactly th.  r in [0.10, 0.16] nm, b in [100, 125] degrees.
  angle     p1 = 0, p0 = r1 z, p2 = r2 (sin al, 0, cos al): the angle at p1 is al = |th|.
  distance  p1 = p0 + d u with a unit vector u, d in [0.1, 1] nm.
th runs over THETA_GRID (0, +-pi/2, pi, +-(pi - 1e-3), +-1e-3 and 64 uniform values), DRAWS draws of the other numbers each; every group
of atoms gets its own random proper rotation and an offset of up to 0.5 nm (the sampler mean-centres: nothing lies further out).  One
frame holds all three groups: 9 atoms, the table ANALYTIC_INDEX (a dihedral, an angle and a distance row).

RIGID case: tumbled, shifted images of the 33-atom chain without noise, for tables of any length over random atoms (`mixed_table`: rows
drawn until they are well conditioned in the chain's own positions, which a rigid motion keeps).

MOLECULE frames: the Ala-Gly dipeptide (its torsions, C-alpha distance and the bond angles inside them) and a synthetic 33-atom chain
(`chain_features`: dihedrals, angles and distances along its bonds, interleaved), tumbled, shifted and with Gaussian noise of SIGMA[name]
on every coordinate.  Only frames in which every bond inside a feature is at least MIN_BOND long and every bond angle inside a dihedral has
sin >= MIN_SIN are kept: below that a dihedral stops being a function a perturbation of 1e-7 leaves alone (its error grows as
1 / (bond sin)), and comparing two precisions there tests the case, not the code.  `molecule_case` reports the share of drawn frames the rule
drops; test_intcoord_host.py asserts it is at most 5 %.

TORSION_TOL_RAD and DIST_TOL_NM are MEASURED (test_intcoord_host.py::test_tolerances_are_four_times_the_float32_models_deviation): four
times the worst deviation of a float32 numpy model of the kernel's arithmetic (`kernel_model`) from the analytic values and from the fp64
specification over every case here, rounded up to one significant digit.
"""
import functools

import numpy as np

from _superpose_cases import random_rotations
from _traj_molecules import dipeptide
from jamun_amd import synth

# measured: the float32 model's worst deviation is 3.98e-7 rad (angles, dihedrals, cos and sin; an analytic dihedral) and 1.31e-7 nm
# (distances; atoms ~2 nm apart in the rigid 33-atom chain); four times that, rounded up to one significant digit
TORSION_TOL_RAD = 2e-6
DIST_TOL_NM = 6e-7

SIGMA = {"dipeptide": 0.04, "chain33": 0.02}  # nm: see `molecule_case` for why the chain gets half the sampler's noise level
MIN_BOND = 0.05   # nm
MIN_SIN = 0.2
DRAWS = 4
N_MOLECULE_FRAMES = 400

_uniform = -np.pi + (np.arange(64) + 0.5) * (2.0 * np.pi / 64)
THETA_GRID = np.concatenate([[0.0, np.pi / 2, -np.pi / 2, np.pi, np.pi - 1e-3, -(np.pi - 1e-3), 1e-3, -1e-3], _uniform])
ANALYTIC_INDEX = np.array([[0, 1, 2, 3], [4, 5, 6, -1], [7, 8, -1, -1]], dtype=np.int32)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)  # (cached and shared among the tests: read only)
    return a


def wrapped(a, b) -> np.ndarray:
    """The difference of two dihedrals on the circle, in [-pi, pi): omega sits on the branch cut, a raw difference is never taken."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d + np.pi) % (2.0 * np.pi) - np.pi


def kinds(index: np.ndarray) -> np.ndarray:
    """Leading non-negative entries of each row of an index table: 2 distance, 3 angle, 4 dihedral."""
    return np.cumprod(np.asarray(index) >= 0, axis=1).sum(axis=1)


def deviation(got, want, index, cossin: bool = False):
    """``(angular, distance)``: the worst deviation of ``got`` from ``want`` ([T, W] both) over the angle / dihedral columns (dihedrals
    wrapped; cos / sin values directly) and over the distance columns (with cossin the constant 0 beside a distance too)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    k = kinds(index)
    ang, dist = 0.0, 0.0
    for j in range(len(k)):
        cols = (2 * j, 2 * j + 1) if cossin else (j,)
        for c in cols:
            if got.shape[0] == 0:
                continue
            d = got[:, c] - want[:, c]
            if k[j] == 4 and not cossin:
                d = wrapped(got[:, c], want[:, c])
            assert np.isfinite(d).all(), (j, c)
            if k[j] == 2:
                dist = max(dist, float(np.abs(d).max()))
            else:
                ang = max(ang, float(np.abs(d).max()))
    return ang, dist


def with_cossin(values: np.ndarray, index: np.ndarray) -> np.ndarray:
    """[T, F] angles and distances -> the [T, 2 F] layout of cossin: (cos, sin) of an angle or dihedral, (d, 0) of a distance."""
    k = kinds(index)
    out = np.empty((values.shape[0], 2 * values.shape[1]))
    for j in range(values.shape[1]):
        out[:, 2 * j] = values[:, j] if k[j] == 2 else np.cos(values[:, j])
        out[:, 2 * j + 1] = 0.0 if k[j] == 2 else np.sin(values[:, j])
    return out


# ---- analytic cases ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def analytic_case():
    """``(frames float64 [T, 9, 3], expected float64 [T, 3])``: dihedral th, angle |th|, distance d per frame; index table ANALYTIC_INDEX."""
    rng = np.random.RandomState(20261019)
    th = np.repeat(THETA_GRID, DRAWS)
    T = th.shape[0]
    r = rng.uniform(0.10, 0.16, size=(T, 5))
    b = np.deg2rad(rng.uniform(100.0, 125.0, size=(T, 2)))
    zero = np.zeros(T)
    dih = np.stack([np.stack([r[:, 0] * np.sin(b[:, 0]), zero, r[:, 0] * np.cos(b[:, 0])], -1),
                    np.zeros((T, 3)),
                    np.stack([zero, zero, r[:, 1]], -1),
                    np.stack([r[:, 2] * np.sin(b[:, 1]) * np.cos(th), r[:, 2] * np.sin(b[:, 1]) * np.sin(th), r[:, 1] - r[:, 2] * np.cos(b[:, 1])], -1)], 1)
    al = np.abs(th)
    ang = np.stack([np.stack([zero, zero, r[:, 3]], -1), np.zeros((T, 3)), np.stack([r[:, 4] * np.sin(al), zero, r[:, 4] * np.cos(al)], -1)], 1)
    d = rng.uniform(0.1, 1.0, size=T)
    u = rng.randn(T, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.stack([np.zeros((T, 3)), d[:, None] * u], 1)
    groups = []
    for g in (dih, ang, dist):
        rot = random_rotations(rng, T)
        shift = rng.randn(T, 1, 3)
        shift *= rng.uniform(0.0, 0.5, size=(T, 1, 1)) / np.linalg.norm(shift, axis=2, keepdims=True)  # |shift| <= 0.5 nm
        g = g - g.mean(axis=1, keepdims=True)  # (the group about the origin, so that shift is what lies between it and the origin)
        groups.append(np.einsum("fab,fib->fia", rot, g) + shift)
    return _frozen(np.concatenate(groups, axis=1)), _frozen(np.stack([th, al, d], axis=1))


# ---- molecule cases ----------------------------------------------------------------------------------------------------------------------

def chain_features(mol: dict, n_each: int):
    """An index table along the bonds of ``mol``: up to ``n_each`` dihedrals i-j-k-l, angles i-j-k and distances i-j, interleaved
    (dihedral, angle, distance, dihedral, ...), in the order the bond list gives; only angles and dihedrals whose bond angles in
    ``mol["pos"]`` itself have sin >= 0.7 (the noise then takes few of them below MIN_SIN)."""
    pos = mol["pos"].numpy().astype(np.float64)
    bonds = [(int(a), int(b)) for a, b in mol["bonds"].T.tolist()]
    nb = {}
    for a, b in bonds:
        nb.setdefault(a, []).append(b)
        nb.setdefault(b, []).append(a)

    def sin_at(i, j, k):
        a, b = pos[i] - pos[j], pos[k] - pos[j]
        return np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))

    angles = [(i, j, k) for j in sorted(nb) for i in nb[j] for k in nb[j] if i < k and sin_at(i, j, k) >= 0.7]
    dihedrals = [(i, j, k, l) for j, k in bonds for i in nb[j] if i != k for l in nb[k] if l != j and l != i
                 and sin_at(i, j, k) >= 0.7 and sin_at(j, k, l) >= 0.7]
    rows = []
    for t in range(n_each):
        for group in (dihedrals, angles, bonds):
            if t < len(group):
                rows.append(tuple(group[t]) + (-1,) * (4 - len(group[t])))
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


def dipeptide_features():
    """The dipeptide's torsions (phi, psi, omega: no side chain beyond CB), the bond angles inside them, and its C-alpha distance."""
    from jamun_amd.features import ca_distance_indices, torsion_indices

    mol = dipeptide()
    tors, _ = torsion_indices(mol, backbone=True, sidechain=True)
    ca, _ = ca_distance_indices(mol)
    angles = sorted({tuple(row[s : s + 3]) for row in tors.tolist() for s in (0, 1)})
    return np.concatenate([tors, np.array([a + (-1,) for a in angles], dtype=np.int32), ca]).astype(np.int32)


def _well_conditioned(frames: np.ndarray, index: np.ndarray) -> np.ndarray:
    """Per frame: every bond inside a feature >= MIN_BOND, every bond angle inside a dihedral with sin >= MIN_SIN (fp64)."""
    ok = np.ones(frames.shape[0], dtype=bool)
    for row, k in zip(index.tolist(), kinds(index)):
        p = [frames[:, v, :] for v in row[:k]]
        b = [p[i + 1] - p[i] for i in range(k - 1)]
        for v in b:
            ok &= np.linalg.norm(v, axis=1) >= MIN_BOND
        if k == 4:
            for u, v in ((b[0], b[1]), (b[1], b[2])):
                ok &= np.linalg.norm(np.cross(u, v), axis=1) >= MIN_SIN * np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1)
    return ok


@functools.lru_cache(maxsize=None)
def molecule_case(name: str):
    """``(frames float32 [T, n, 3], index int32 [F, 4], dropped share)`` of "dipeptide" or "chain33": N_MOLECULE_FRAMES tumbled noisy
    images of the molecule, less the frames the conditioning rule drops.

    The dipeptide gets the sampler's noise level, 0.04 nm on every coordinate; the rule then drops 4.5 % of its frames (three dihedrals).
    The rule costs 2 to 3 % of the frames PER DIHEDRAL at that level (a 0.15 nm bond's direction scatters by 0.4 rad), so the chain's table of
    18 rows with six dihedrals, which is there to cross a feature tile of the kernel, would lose 14 %; the chain gets 0.02 nm (the saved
    frames are the DENOISED xhat: less than the noise level is what they carry) and loses under 1 %."""
    if name == "dipeptide":
        mol, index, seed = dipeptide(), dipeptide_features(), 11
    elif name == "chain33":
        mol = synth.random_chain(33, seed=33)
        index, seed = chain_features(mol, 6), 33
    else:
        raise KeyError(name)
    rng = np.random.RandomState(seed)
    pos = mol["pos"].numpy().astype(np.float64)
    pos = pos - pos.mean(axis=0)
    T = N_MOLECULE_FRAMES
    shift = rng.randn(T, 1, 3)
    shift *= rng.uniform(0.0, 0.5, size=(T, 1, 1)) / np.linalg.norm(shift, axis=2, keepdims=True)
    frames = np.einsum("fab,ib->fia", random_rotations(rng, T), pos) + shift + SIGMA[name] * rng.randn(T, pos.shape[0], 3)
    frames = frames.astype(np.float32)
    ok = _well_conditioned(frames.astype(np.float64), index)
    return _frozen(np.ascontiguousarray(frames[ok])), _frozen(index), 1.0 - float(ok.mean())


def mixed_table(pos: np.ndarray, n_feat: int, seed: int = 0) -> np.ndarray:
    """``n_feat`` rows over the atoms of ``pos [n, 3]``: distance, angle and dihedral rows interleaved, distinct random atoms in each row,
    drawn again until consecutive atoms of the row are at least 0.1 nm apart and the angles inside it have sin >= 0.7 in ``pos``
    (rigid images of ``pos`` then are as well conditioned as the analytic cases)."""
    rng = np.random.RandomState(1000 + seed)
    pos = np.asarray(pos, dtype=np.float64)
    rows = []
    while len(rows) < n_feat:
        k = 2 + len(rows) % 3
        row = [int(v) for v in rng.choice(pos.shape[0], size=k, replace=False)]
        b = [pos[row[i + 1]] - pos[row[i]] for i in range(k - 1)]
        if min(np.linalg.norm(v) for v in b) < 0.1:
            continue
        if any(np.linalg.norm(np.cross(u, v)) < 0.7 * np.linalg.norm(u) * np.linalg.norm(v) for u, v in zip(b, b[1:])):
            continue
        rows.append(tuple(row) + (-1,) * (4 - k))
    return np.array(rows, dtype=np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def rigid_case(T: int = 257):
    """``(frames float32 [T, 33, 3], pos float64 [33, 3])``: rigid tumbled, shifted images of the 33-atom chain, no noise."""
    rng = np.random.RandomState(257)
    pos = synth.random_chain(33, seed=33)["pos"].numpy().astype(np.float64)
    pos = pos - pos.mean(axis=0)
    shift = rng.uniform(-0.3, 0.3, size=(T, 1, 3))
    return _frozen((np.einsum("fab,ib->fia", random_rotations(rng, T), pos) + shift).astype(np.float32)), _frozen(pos)


# ---- a float32 numpy model of k_internal_coords: differences first, fp32 products and sums in the kernel's order, np.arctan2 in float32

_f = np.float32


def _dot32(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross32(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _pair32(y, x, cossin):
    if not cossin:
        return np.arctan2(y, x), np.zeros_like(x)
    m = np.maximum(np.abs(x), np.abs(y))
    zero = m == 0
    ms = np.where(zero, _f(1.0), m)
    xs, ys = x / ms, y / ms
    r = np.sqrt(xs * xs + ys * ys)
    return np.where(zero, np.copysign(_f(1.0), x), xs / r), np.where(zero, _f(0.0), ys / r)


def kernel_model(frames: np.ndarray, index: np.ndarray, cossin: bool = False) -> np.ndarray:
    """float32 [T, W] computed the way the kernel computes it, one numpy lane per frame (in-range rows of finite frames only)."""
    x = np.asarray(frames, dtype=np.float32)
    out = np.empty((x.shape[0], index.shape[0] * (2 if cossin else 1)), dtype=np.float32)
    for j, (row, k) in enumerate(zip(index.tolist(), kinds(index))):
        p = [[x[:, v, c] for c in range(3)] for v in row[:k]]
        sub = lambda a, b: [a[c] - b[c] for c in range(3)]
        if k == 2:
            d = sub(p[1], p[0])
            v0, v1 = np.sqrt(_dot32(d, d)), np.zeros(x.shape[0], dtype=np.float32)
        elif k == 3:
            a, b = sub(p[0], p[1]), sub(p[2], p[1])
            c = _cross32(a, b)
            v0, v1 = _pair32(np.sqrt(_dot32(c, c)), _dot32(a, b), cossin)
        else:
            b1, b2, b3 = sub(p[1], p[0]), sub(p[2], p[1]), sub(p[3], p[2])
            c1, c2 = _cross32(b2, b3), _cross32(b1, b2)
            v0, v1 = _pair32(_dot32(b1, c1) * np.sqrt(_dot32(b2, b2)), _dot32(c1, c2), cossin)
        assert v0.dtype == np.float32 and v1.dtype == np.float32
        if cossin:
            out[:, 2 * j], out[:, 2 * j + 1] = v0, v1
        else:
            out[:, j] = v0
    return out


# ---- stand-ins for the callback tests ----------------------------------------------------------------------------------------------------

def tumbling_batches(mol: dict, device, chains: int, T: int, n_batches: int, seed: int, sigma: float = 0.02):
    """Samples as `unbatch_samples` hands them out ([n, T, 3] views of one [T, sum N, 3] tensor on ``device``): tumbling noisy images of pos."""
    import torch

    rng = np.random.RandomState(seed)
    pos = mol["pos"].numpy().astype(np.float64)
    n = pos.shape[0]
    out = []
    for _ in range(n_batches):
        traj = np.empty((T, chains * n, 3), dtype=np.float32)
        for c in range(chains):
            traj[:, c * n : (c + 1) * n] = (np.einsum("fab,ib->fia", random_rotations(rng, T), pos) + rng.uniform(-0.3, 0.3, size=(T, 1, 3))
                                            + sigma * rng.randn(T, n, 3))
        traj = torch.from_numpy(traj).to(device)
        out.append([{"dataset_label": "m", "atom_type_index": mol["atom_type_index"], "xhat_traj": traj[:, c * n : (c + 1) * n].permute(1, 0, 2)}
                    for c in range(chains)])
    return out


def run_callback(cb, batches, device):
    from _superpose_cases import CaseSampler

    smp = CaseSampler(device)
    cb.on_sample_start(smp)
    for b in batches:
        cb.on_after_sample_batch(b, smp)
        cb.flush()
    cb.on_sample_end(smp)
    return cb
