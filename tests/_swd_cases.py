"""What test_swd_host.py and test_gpu_swd.py share: the brute force behind W2^2, key tables with every special value, the shapes of the
W2^2 cases, and the fixture of the meter with the measured sensitivity of its distances.

THE METER FIXTURE.  The Ala-Gly dipeptide with driven torsions of `_tica_cases` (one phi, one psi: 4 descriptor columns): `REFERENCE_T`
reference frames and one batch of two chains of `CHAIN_T` frames, so that the joined trajectory's cut 400 falls inside the second chain.

THE TOLERANCE OF THE DEVICE PATH.  The device forms the dihedral, ``cosf`` and ``sinf`` in fp32 where the host path rounds float64 values
to fp32, so a descriptor differs from the host's in its last places.  The rounding bound of such a descriptor is `DESCRIPTOR_EPS` = 4e-7:
the worst deviation of a float32 numpy model of the kernel's arithmetic from the fp64 specification (cos and sin of dihedrals included),
measured on the CPU in `_intcoord_cases` (3.98e-7).  `measure_sensitivity` moves every float32 descriptor of the host path (chains and
reference) by that much with random signs, 16 draws, and records the largest change of any ``ws_distance``.  `OBSERVED` is that
measurement; `TOLERANCE` is ten times it (test_swd_host.py repeats the measurement and holds the constant to it within a factor 2).
For scale: a shift of every key by at most e moves each W2, and with it the distance, by at most e (the triangle inequality of W2 and of
the root mean square), and a key moves by at most sqrt(4) * 4e-7 = 8e-7 (4 unit columns): the tolerance may not exceed that bound by much,
and random signs leave a fraction of it.
"""
import numpy as np
import torch

import _tica_cases as tc

W2SQ_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (6, 4), (100, 257), (257, 100)]


def w2sq_bound(n: int, m: int) -> float:
    return (n + m) * 2.0 ** -52


def sorted_columns(L: int, n: int, seed: int) -> np.ndarray:
    """float32 [L, n], every row ascending."""
    return np.sort(np.random.RandomState(seed).randn(L, n).astype(np.float32), axis=1)


def brute_w2sq(u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """The quantile integral on the grid of n m cells written out: every cell of u repeated m times against every cell of v repeated n times."""
    n, m = u.shape[1], v.shape[1]
    d = np.repeat(u.astype(np.float64), m, axis=1) - np.repeat(v.astype(np.float64), n, axis=1)
    return np.mean(d * d, axis=1)


def special_keys() -> np.ndarray:
    """float32 in the order `order_image` must give them: -NaN and +NaN excluded, they go last.  -inf, negatives, -denormals, -0, +0,
    +denormals, positives, +inf."""
    bits = np.array([0xFF800000, 0xFF7FFFFF, 0xC0000000, 0xBF800000, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000,
                     0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x40000000, 0x7F7FFFFF, 0x7F800000], dtype=np.uint32)
    return bits.view(np.float32)


def nan_keys() -> np.ndarray:
    """NaNs of both signs, quiet and signalling, with and without payload."""
    return np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)


def key_data(kind: str, L: int, T: int, seed: int = 0) -> np.ndarray:
    """float32 [L, T] of one of the data cases of the sort tests."""
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randn(L, T).astype(np.float32)
    if kind == "sorted":
        return np.sort(rng.randn(L, T).astype(np.float32), axis=1)
    if kind == "reversed":
        return np.array(np.sort(rng.randn(L, T).astype(np.float32), axis=1)[:, ::-1], order="C", copy=True)
    if kind == "equal":
        return np.full((L, T), np.float32(0.25))
    if kind == "ties":
        return rng.randint(-3, 4, size=(L, T)).astype(np.float32)
    if kind == "special":
        table = np.concatenate([special_keys(), nan_keys()])
        return table[rng.randint(0, table.shape[0], size=(L, T))]
    raise ValueError(kind)


# ---- the meter ----------------------------------------------------------------------------------------------------------------------------

REFERENCE_T, CHAIN_T = 600, 250
DESCRIPTOR_EPS = 4.0e-7  # see the module docstring
OBSERVED = 5.02e-8  # the largest change of a ws_distance `measure_sensitivity` saw on this fixture with 16 draws
TOLERANCE = 10.0 * OBSERVED


def meter_fixture(mol: dict, device):
    """(reference frames [REFERENCE_T, 10, 3] as a CPU tensor, one batch of two chains of CHAIN_T frames on ``device``)."""
    return torch.from_numpy(np.array(tc.dipeptide_torsion_frames(mol, REFERENCE_T, 500))), tc.torsion_batches(mol, device, 2, CHAIN_T, 1, seed=600)


def measure_sensitivity(x_ref: np.ndarray, x_chains, proj: np.ndarray, cuts_of, draws: int = 16) -> float:
    """The largest change of ``sliced_wasserstein_host(chain[:k], reference)`` over the chains, the joined trajectory and every cut ``k`` of
    ``cuts_of(T)`` when every descriptor moves by +-`DESCRIPTOR_EPS` with random signs."""
    from jamun_amd import swd

    eps = np.float32(DESCRIPTOR_EPS)
    clouds = list(x_chains) + [np.concatenate(x_chains)]

    def curve(ref, cl):
        return np.array([swd.sliced_wasserstein_host(x[:k], ref, proj) for x in cl for k in cuts_of(x.shape[0])])

    base = curve(x_ref, clouds)
    worst = 0.0
    for seed in range(draws):
        rng = np.random.RandomState(2000 + seed)
        move = lambda x: (x + np.where(rng.rand(*x.shape) < 0.5, -eps, eps)).astype(np.float32)
        worst = max(worst, float(np.abs(curve(move(x_ref), [move(x) for x in clouds]) - base).max()))
    return worst
