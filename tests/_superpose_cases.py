"""Cases and an independent fp64 reference for the superposition tests (test_superpose_host.py, test_gpu_superpose.py).

The reference is Horn's quaternion method through ``numpy.linalg.eigh`` in float64: NOT the product's host path (Kabsch by SVD) and not
the kernel's eigen-solver (Jacobi in fp32), so agreement between any two of the three is evidence.  Besides the aligned frames and the
RMSD it returns ``g``, the gap between the two largest eigenvalues of the 4x4 matrix over the largest: the condition of the rotation.  A
perturbation dN of the matrix turns the eigenvector by ~ |dN| / (g lambda_max), so a frame's coordinates are comparable between two
methods only where g is well above the arithmetic's relative error; where g = 0 (rank-deficient covariance: one or two atoms, collinear
atoms) the rotation about the free axis is arbitrary and only the RMSD and the shape of the aligned frame are defined.

Molecules (issue): the Ala-Gly dipeptide and random chains of 1, 2, 3, 4, 10, 33, 166 atoms; 300 atoms besides, for the kernel's second
reference tile (256 atoms per tile).  Frames are built from ``pos`` in five ways, all seeded: `noisy` random proper rotations + translations
up to 1 nm + Gaussian noise of sigma = 0.04 nm; `identity`; `turn180` exact half turns about x, y, z (sign flips: exact in fp32) and
about a random axis; `rigid` a rotated and translated image without noise; `mirror` the point reflection -pos, rotated.

COORD_MOLECULES are compared on coordinates in EVERY frame of every kind; RANK_DEFICIENT (n <= 2 and a collinear chain) on RMSD and
pairwise distances only.  A mirror image is a different molecule only if the molecule is chiral, which takes four atoms out of a plane:
the 3-atom chain is planar, its mirror image is a half turn about the plane's normal away (RMSD 0, still a unique rotation), so
"the mirror image does not come back" is asserted for CHIRAL molecules (n >= 4) and the 3-atom chain's mirror frames are compared like
all its other frames.
"""
import functools

import numpy as np

from _switch_cases import RMSD_TOL_NM, SIGMA  # noqa: F401  (1e-5 nm, the project's bound; 0.04 nm, the noise level of the sampler)
from jamun_amd import synth

CHAIN_SIZES = (1, 2, 3, 4, 10, 33, 166)
COORD_MOLECULES = ("dipeptide", "chain3", "chain4", "chain10", "chain33", "chain166", "chain300")
CHIRAL_MOLECULES = tuple(m for m in COORD_MOLECULES if m != "chain3")
RANK_DEFICIENT = ("chain1", "chain2", "line5")
KINDS = ("noisy", "identity", "turn180", "rigid", "mirror")
N_NOISY = 24

# Premise 1: every frame of COORD_MOLECULES x KINDS has g >= G_FLOOR.  The smallest is 0.034 (chain3, a noisy frame: three atoms 0.15 nm
# apart under 0.04 nm of noise come close to a line); the mirror frames, whose gap is 2 (s2 - s3) / (s1 + s2 - s3) of the covariance's
# singular values, have g >= 0.11, every other frame g >= 0.13.  fp32 perturbs the 4x4 matrix by ~1e-6 of its norm (sums of up to 300
# products), which turns the eigenvector by ~1e-6 / g <= 3e-5 rad at the floor: on chain3's lever of 0.2 nm that is 6e-6 nm in the worst
# case and a tenth of it typically, so the floor is where the coordinate comparison at RMSD_TOL_NM stops being safe, and no lower.
G_FLOOR = 0.03
# Premise 2: the largest deviation of the float32 model of the kernel (`kernel_model`) from the fp64 reference over the same frames, as
# printed by test_superpose_host.py::test_float32_model_of_the_kernel_stays_within_half_the_bound (nm): coordinates (per-frame RMSD to the
# reference's aligned frame; chain166, a mirror frame) and rmsd (chain300, a rigid image).  Both have to stay below RMSD_TOL_NM / 2 = 5e-6.
MODEL_DEV_NM = {"coords": 9.3e-7, "rmsd": 5.7e-7}


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)  # (cached and shared among the tests: read only)
    return a


@functools.lru_cache(maxsize=None)
def molecule_pos(name: str) -> np.ndarray:
    """float32 [n, 3] positions (nm) of a named case molecule."""
    if name == "dipeptide":
        pos = synth.ag_dipeptide()["pos"]
    elif name.startswith("chain"):
        n = int(name[5:])
        pos = synth.random_chain(n, seed=n)["pos"]
    elif name == "line5":  # five atoms on one line, 0.15 nm apart, in a general direction
        d = np.array([0.36, -0.48, 0.8])
        return _frozen((np.arange(5)[:, None] * 0.15 * d[None, :] + np.array([0.3, -0.2, 0.1])).astype(np.float32))
    else:
        raise KeyError(name)
    return _frozen(np.array(pos.detach().cpu().numpy() if hasattr(pos, "detach") else pos, dtype=np.float32))


def random_rotations(rng: np.random.RandomState, k: int) -> np.ndarray:
    """k proper rotations [k, 3, 3], uniform (normalised Gaussian quaternions)."""
    q = rng.randn(k, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def _seed(name: str, kind: str) -> int:
    return 1000 * (sorted(COORD_MOLECULES + RANK_DEFICIENT).index(name) + 1) + KINDS.index(kind)


@functools.lru_cache(maxsize=None)
def frames_of(name: str, kind: str, k: int = N_NOISY) -> np.ndarray:
    """float32 [F, n, 3] frames of one kind built from the molecule's pos (F = k for `noisy`, 4 for `turn180`, 1 for `identity`, else 6)."""
    pos = molecule_pos(name).astype(np.float64)
    rng = np.random.RandomState(_seed(name, kind))
    if kind == "identity":
        out = pos[None]
    elif kind == "turn180":
        a = rng.randn(3)
        a /= np.linalg.norm(a)
        half = 2.0 * np.outer(a, a) - np.eye(3)  # half turn about a
        out = np.stack([pos * np.array([1.0, -1.0, -1.0]), pos * np.array([-1.0, 1.0, -1.0]), pos * np.array([-1.0, -1.0, 1.0]), pos @ half.T])
    else:
        F = k if kind == "noisy" else 6
        rot = random_rotations(rng, F)
        shift = rng.uniform(-1.0, 1.0, size=(F, 1, 3)) / np.sqrt(3.0)  # |shift| <= 1 nm
        base = -pos if kind == "mirror" else pos
        out = np.einsum("fab,ib->fia", rot, base) + shift
        if kind == "noisy":
            out = out + SIGMA * rng.randn(*out.shape)
    return _frozen(np.array(out, dtype=np.float32, order="C"))


def all_frames(name: str) -> np.ndarray:
    """Every kind of frame of a molecule in one float32 [F, n, 3] array, in the order of KINDS."""
    return np.concatenate([frames_of(name, kind) for kind in KINDS])


def kind_slices(name: str) -> dict:
    out, at = {}, 0
    for kind in KINDS:
        F = frames_of(name, kind).shape[0]
        out[kind] = slice(at, at + F)
        at += F
    return out


def horn_reference(frames: np.ndarray, ref: np.ndarray):
    """fp64 reference: ``(aligned [F, n, 3], rmsd [F], g [F])`` by Horn's quaternion method with numpy.linalg.eigh."""
    x = np.asarray(frames, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    cx = x.mean(axis=1, keepdims=True)
    cr = r.mean(axis=0)
    xc, rc = x - cx, r - cr
    S = np.einsum("fia,ib->fab", xc, rc)
    N = np.empty((x.shape[0], 4, 4))
    N[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    N[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    N[:, 2, 2] = -S[:, 0, 0] + S[:, 1, 1] - S[:, 2, 2]
    N[:, 3, 3] = -S[:, 0, 0] - S[:, 1, 1] + S[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    lam, vec = np.linalg.eigh(N)  # ascending
    q = vec[:, :, 3]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)], -1),
                    np.stack([2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)], -1),
                    np.stack([2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], -1)], 1)
    aligned = np.einsum("fab,fib->fia", rot, xc) + cr
    rmsd = np.sqrt(((aligned - r) ** 2).sum(axis=(1, 2)) / x.shape[1])
    top = np.where(lam[:, 3] > 0, lam[:, 3], 1.0)
    g = np.where(lam[:, 3] > 0, (lam[:, 3] - lam[:, 2]) / top, 0.0)
    return aligned, rmsd, g


@functools.lru_cache(maxsize=None)
def case(name: str):
    """``(pos, frames, (aligned, rmsd, g))`` of a molecule: all its frames and their fp64 reference, computed once, shared, read only."""
    pos, frames = molecule_pos(name), _frozen(all_frames(name))
    return pos, frames, tuple(_frozen(a) for a in horn_reference(frames, pos))


def frame_rmsd(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Per frame sqrt(mean_i |a_i - b_i|^2) of two [F, n, 3] arrays, in float64."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.sqrt((d * d).sum(axis=(1, 2)) / d.shape[1])


def pair_distances(x: np.ndarray) -> np.ndarray:
    """[F, n, n] distances between the atoms of every frame, in float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.linalg.norm(x[:, :, None, :] - x[:, None, :, :], axis=-1)


# ---- a float32 numpy model of k_superpose_frames: the same centring (fp64 centroid sums, fp32 everything else), the same covariance order,
# ---- the same six cyclic Jacobi sweeps with the same formulas, the same selection and normalisation, the same RMSD pass

SWEEPS = 6
_f = np.float32


def _rotate(A, V, p, q):
    app, aqq, apq = A[p][p], A[q][q], A[p][q]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        theta = (aqq - app) / (_f(2.0) * apq)
        root = np.sqrt(theta * theta + _f(1.0))
        t = np.where(theta < 0, _f(-1.0), _f(1.0)) / (np.abs(theta) + root)
    t = np.where(apq == 0, _f(0.0), t).astype(np.float32)
    c = _f(1.0) / np.sqrt(t * t + _f(1.0))
    s = t * c
    A[p][p] = app - t * apq
    A[q][q] = aqq + t * apq
    A[p][q] = A[q][p] = np.zeros_like(apq)
    for r in range(4):
        if r != p and r != q:
            x, y = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * x - s * y
            A[r][q] = A[q][r] = s * x + c * y
    for r in range(4):
        x, y = V[r][p], V[r][q]
        V[r][p] = c * x - s * y
        V[r][q] = s * x + c * y


def kernel_model(frames: np.ndarray, ref: np.ndarray):
    """``(aligned float32 [F, n, 3], rmsd float32 [F])`` computed the way the kernel computes them, one numpy lane per frame."""
    x = np.asarray(frames, dtype=np.float32)
    r = np.asarray(ref, dtype=np.float32)
    F, n = x.shape[0], x.shape[1]
    cr = (r.astype(np.float64).sum(axis=0) / n).astype(np.float32)
    cx = (x.astype(np.float64).sum(axis=1) / n).astype(np.float32)  # [F, 3]
    S = [[np.zeros(F, dtype=np.float32) for _ in range(3)] for _ in range(3)]
    for i in range(n):
        xc = x[:, i, :] - cx
        rc = r[i] - cr
        for a in range(3):
            for b in range(3):
                S[a][b] = S[a][b] + xc[:, a] * rc[b]
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = S
    A = [[None] * 4 for _ in range(4)]
    A[0][0] = sxx + syy + szz
    A[1][1] = sxx - syy - szz
    A[2][2] = syy - sxx - szz
    A[3][3] = szz - sxx - syy
    A[0][1] = A[1][0] = syz - szy
    A[0][2] = A[2][0] = szx - sxz
    A[0][3] = A[3][0] = sxy - syx
    A[1][2] = A[2][1] = sxy + syx
    A[1][3] = A[3][1] = szx + sxz
    A[2][3] = A[3][2] = syz + szy
    V = [[np.full(F, 1.0 if i == j else 0.0, dtype=np.float32) for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate(A, V, p, q)
    hi01, hi23 = A[1][1] > A[0][0], A[3][3] > A[2][2]
    t01, t23 = np.where(hi01, A[1][1], A[0][0]), np.where(hi23, A[3][3], A[2][2])
    hi = t23 > t01
    quat = [np.where(hi, np.where(hi23, V[k][3], V[k][2]), np.where(hi01, V[k][1], V[k][0])) for k in range(4)]
    qw, qx, qy, qz = quat
    inv = _f(1.0) / np.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw, qx, qy, qz = qw * inv, qx * inv, qy * inv, qz * inv
    two, one = _f(2.0), _f(1.0)
    R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qw * qz), two * (qx * qz + qw * qy)],
         [two * (qx * qy + qw * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qw * qx)],
         [two * (qx * qz - qw * qy), two * (qy * qz + qw * qx), one - two * (qx * qx + qy * qy)]]
    out = np.empty_like(x)
    acc = np.zeros(F, dtype=np.float32)
    for i in range(n):
        xc = x[:, i, :] - cx
        y = [(R[a][0] * xc[:, 0] + R[a][1] * xc[:, 1] + R[a][2] * xc[:, 2]) + cr[a] for a in range(3)]
        for a in range(3):
            out[:, i, a] = y[a]
        d = [y[a] - r[i, a] for a in range(3)]
        acc = acc + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return out, np.sqrt(acc / _f(n))


# ---- readers of the callback's files (coordinates back in nm / Angstrom thousandths) and the callback's stand-ins

DCD_PREAMBLE = 276  # bytes of a save_dcd file in front of the coordinate records: header, title block, atom count


def read_dcd_nm(path: str, n_atoms: int) -> np.ndarray:
    """float32 [T, n, 3] frames of a `pdb.save_dcd` file, as stored (Angstrom) divided by 10 in float64 -> nm."""
    raw = open(path, "rb").read()[DCD_PREAMBLE:]
    rec = np.dtype([("a", "<i4"), ("v", "<f4", (n_atoms,)), ("b", "<i4")])
    recs = np.frombuffer(raw, dtype=rec).reshape(-1, 3)
    assert (recs["a"] == 4 * n_atoms).all() and (recs["b"] == 4 * n_atoms).all()
    return np.transpose(recs["v"].astype(np.float64), (0, 2, 1)) / 10.0


def read_pdb_milli_angstrom(path: str, n_atoms: int) -> np.ndarray:
    """int64 [T, n, 3]: the coordinate fields of every ATOM record of a `pdb.save_pdb` file in thousandths of an Angstrom (the format's
    resolution: fields of %8.3f), so that two files are compared in whole units."""
    vals = []
    for line in open(path):
        if line.startswith("ATOM"):
            vals.append([int(round(float(line[30 + 8 * c : 38 + 8 * c]) * 1000.0)) for c in range(3)])
    return np.array(vals, dtype=np.int64).reshape(-1, n_atoms, 3)


def milli_angstrom(frames_nm: np.ndarray) -> np.ndarray:
    """What `read_pdb_milli_angstrom` reads back from frames written by `pdb.save_pdb`: round(fp32(x * 10) * 1000)."""
    return np.rint((np.asarray(frames_nm, dtype=np.float32) * np.float32(10.0)).astype(np.float64) * 1000.0).astype(np.int64)


class CaseSampler:
    is_global_zero = True; world_size = 1; global_step = 0

    def __init__(self, device):
        self.device = device
