"""Cases and an independent fp64 reference for the denoising-evaluation tests (test_denoise_host.py, test_gpu_denoise.py).

Molecules: the Ala-Gly dipeptide (10 atoms) and random chains of 1, 2, 3, 17, 64, 65, 166 atoms (64 / 65: half of k_noise_align's 128
threads and one over; 166: more atoms than threads), and five atoms on a line.  DEGENERATE (one atom, two atoms, the line) have a
rank-deficient covariance: some optimal rotation is as good as another, so their RMSD is compared and their coordinates are not.  Two
batches: `ragged` mixes every molecule, one graph each, in an order that puts the degenerate ones between the others; `dense` is 70 graphs
of the 17-atom chain.  Noise is seeded numpy; sigma is SIGMA (0.04 nm) and 0.4 nm.

The reference is a numpy float64 restatement of the two pieces of the reference package the kernels mirror, which cannot be imported here
(``utils/align.py`` imports torch_scatter):
  * `kabsch_reference`  ``src/jamun/utils/align.py:30-55``  (centroids, covariance H = y_c^T x_c, SVD, R = V U^T, the determinant
                        fix on the last singular direction, t = x_mu - R y_mu, y_aligned = R y + t);
  * `loss_reference`    ``src/jamun/model/denoiser.py:262-281``  (squared error summed over the components, scaled_rmsd =
                        sqrt(.) / (sigma sqrt D), scatter_mean over each graph, times loss_weight and 1 / c_out^2).
`horn_gap` is the conditioning of a graph's rotation, from `_superpose_cases.horn_reference` (an eigh of Horn's matrix: a third method).
"""
import functools

import numpy as np

import _superpose_cases as sp
from _switch_cases import RMSD_TOL_NM, SIGMA  # noqa: F401  (1e-5 nm, the project's bound; 0.04 nm)
from jamun_amd import synth

SIGMAS = (SIGMA, 0.4)
G_FLOOR = sp.G_FLOOR  # tests/_superpose_cases.py:37-39: below it the coordinates of two methods are no longer comparable at RMSD_TOL_NM
CHAINS = (1, 2, 3, 17, 64, 65, 166)
RAGGED = ("dipeptide", "chain1", "chain17", "chain2", "chain64", "line5", "chain65", "chain3", "chain166")
DEGENERATE = ("chain1", "chain2", "line5")
DENSE = ("chain17",) * 70
BATCHES = {"ragged": RAGGED, "dense": DENSE}
NOISE_SEED = {"ragged": 5, "dense": 6}  # (a graph below G_FLOOR: change the seed here, not the tolerance)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def batch(kind: str):
    """``(x float32 [N, 3], noise float32 [N, 3], ptr int32 [W + 1], names)`` of a batch, shared and read only.  x is shifted by up to
    1 nm per graph, so that centring has something to do."""
    names = BATCHES[kind]
    rng = np.random.RandomState(NOISE_SEED[kind])
    xs, ptr = [], [0]
    for nm in names:
        pos = sp.molecule_pos(nm)  # (chain n: synth.random_chain(n, seed=n))
        xs.append((pos.astype(np.float64) + rng.uniform(-1.0, 1.0, size=(1, 3)) / np.sqrt(3.0)).astype(np.float32))
        ptr.append(ptr[-1] + pos.shape[0])
    x = np.concatenate(xs)
    noise = rng.randn(*x.shape).astype(np.float32)
    return _frozen(x), _frozen(noise), _frozen(np.asarray(ptr, dtype=np.int32)), names


def graphs(ptr):
    return [(g, int(ptr[g]), int(ptr[g + 1])) for g in range(len(ptr) - 1)]


# ---- the fp64 restatements ----------------------------------------------------------------------------------------------------------

def kabsch_reference(y: np.ndarray, x: np.ndarray, ptr) -> np.ndarray:
    """``align.py:30-55`` in float64, graph by graph: the aligned y."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    out = np.empty_like(y)
    for g, lo, hi in graphs(ptr):
        if hi == lo:
            continue
        yg, xg = y[lo:hi], x[lo:hi]
        x_mu, y_mu = xg.mean(axis=0), yg.mean(axis=0)                 # :31-32
        x_c, y_c = xg - x_mu, yg - y_mu                               # :34-35
        H = np.einsum("Ni,Nj->ij", y_c, x_c)                          # :39
        U, _, VH = np.linalg.svd(H)                                   # :42
        R = np.einsum("ki,jk->ij", VH, U)                             # :43  V U^T
        signs = np.eye(3)                                             # :46-48
        signs[2, 2] = np.linalg.det(R)
        R = np.einsum("ki,kk,jk->ij", VH, signs, U)                   # :49  V S U^T
        t = x_mu - R @ y_mu                                           # :52-53
        out[lo:hi] = yg @ R.T + t                                     # :55
    return out


def loss_reference(xhat: np.ndarray, x: np.ndarray, ptr, sigma: float, loss_weight, inv_c_out_sq: float) -> np.ndarray:
    """``denoiser.py:262-281`` in float64 -> [W, 3] (raw_coordinate_loss, scaled_rmsd, coordinate_loss).  sigma is the float32 value
    the reference holds it in (``torch.as_tensor(sigma).to(x.pos)``, :232)."""
    xhat, x = np.asarray(xhat, dtype=np.float64), np.asarray(x, dtype=np.float64)
    D = xhat.shape[-1]                                                # :262
    raw = ((xhat - x) ** 2).sum(axis=-1)                              # :266-267
    scaled = np.sqrt(raw) / (float(np.float32(sigma)) * np.sqrt(D))   # :271
    W = len(ptr) - 1
    out = np.zeros((W, 3))
    for g, lo, hi in graphs(ptr):
        if hi > lo:
            out[g, 0], out[g, 1] = raw[lo:hi].mean(), scaled[lo:hi].mean()  # :275-276
    lw = np.ones(W) if loss_weight is None else np.asarray(loss_weight, dtype=np.float64)
    out[:, 2] = out[:, 0] * lw * float(inv_c_out_sq)                  # :280-281
    return out


def graph_rmsd(a: np.ndarray, b: np.ndarray, ptr) -> np.ndarray:
    """Per graph sqrt(mean_i |a_i - b_i|^2) in float64 (0 for a graph without atoms)."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.array([np.sqrt((d[lo:hi] ** 2).sum() / max(hi - lo, 1)) for _, lo, hi in graphs(ptr)])


def horn_gap(y: np.ndarray, x: np.ndarray, ptr) -> np.ndarray:
    """Per graph the relative gap of the two largest eigenvalues of Horn's matrix of (y, x): 0 where the rotation is not unique."""
    return np.array([float(sp.horn_reference(np.asarray(y[lo:hi])[None], np.asarray(x[lo:hi]))[2][0]) if hi > lo else 0.0 for _, lo, hi in graphs(ptr)])


@functools.lru_cache(maxsize=None)
def aligned_case(kind: str, sigma: float, mean_center: bool = True):
    """``(x_c, y0, y_ref, rmsd_ref, gap)`` of a batch at a noise level: the float32 host mirror's centred x and noisy, centred, NOT yet
    aligned y0 (the kernel's bits, test_gpu_denoise.py asserts that first), and from them in float64 the aligned y, its per-graph RMSD to
    x_c and the gap.  Computed once, shared, read only."""
    from jamun_amd import native_denoise as nd

    x, noise, ptr, _ = batch(kind)
    x_c, y0, _ = nd.noise_align_graphs_host(x, noise, ptr, sigma, mean_center=mean_center, align=False)
    y_ref = kabsch_reference(y0, x_c, ptr)
    return _frozen(x_c), _frozen(y0), _frozen(y_ref), _frozen(graph_rmsd(y_ref, x_c, ptr)), _frozen(horn_gap(y0, x_c, ptr))


# ---- special inputs: y built exactly from x through the noise ------------------------------------------------------------------------
# sigma = 0.5 is a power of two, so sigma * noise is exact: noise = (s - 1) x_c / sigma gives y = x_c + (s - 1) x_c = s x_c per component
# with s in {+1, -1}, exactly (x_c - 2 x_c = -x_c in fp32).  x is centred beforehand and run with mean_center = False.
SPECIAL_SIGMA = 0.5
SPECIAL_SIGNS = {"identity": (1.0, 1.0, 1.0), "mirror": (-1.0, -1.0, -1.0), "turn_x": (1.0, -1.0, -1.0), "turn_y": (-1.0, 1.0, -1.0), "turn_z": (-1.0, -1.0, 1.0)}
SPECIAL_MOLECULES = ("dipeptide", "chain17", "chain166")  # chiral: four atoms out of a plane


@functools.lru_cache(maxsize=None)
def special_case(which: str):
    """``(x, noise, ptr, y_expected_before_alignment)`` for SPECIAL_MOLECULES in one batch."""
    s = np.asarray(SPECIAL_SIGNS[which], dtype=np.float32)
    xs, ptr = [], [0]
    for nm in SPECIAL_MOLECULES:
        p = sp.molecule_pos(nm).astype(np.float64)
        xs.append((p - p.mean(axis=0)).astype(np.float32))
        ptr.append(ptr[-1] + p.shape[0])
    x = np.concatenate(xs)
    noise = ((s - np.float32(1.0)) * x) / np.float32(SPECIAL_SIGMA)
    y0 = x + np.float32(SPECIAL_SIGMA) * noise
    assert np.array_equal(y0, s * x)
    return _frozen(x), _frozen(noise), _frozen(np.asarray(ptr, dtype=np.int32)), _frozen(y0)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

E2E = {"ag4": lambda: [synth.ag_dipeptide()] * 4, "chain17x8": lambda: [synth.random_chain(17, seed=0)] * 8}


class FramesDataset:
    """A dataset of F frames of one molecule, as `evaluate_denoiser` reads it: ``label()``, ``len``, ``[i]`` -> a molecule dict."""

    def __init__(self, mol: dict, label: str, n_frames: int, seed: int = 3, spread_nm: float = 0.02):
        import torch

        g = torch.Generator().manual_seed(seed)
        self._label = label
        self._frames = [dict(mol, pos=mol["pos"] + spread_nm * torch.randn(mol["pos"].shape, generator=g)) for _ in range(n_frames)]

    def label(self):
        return self._label

    def __len__(self):
        return len(self._frames)

    def __getitem__(self, i):
        return self._frames[i]
