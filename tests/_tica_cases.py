"""What test_tica_host.py and test_gpu_tica.py share: the rounding bounds of the three reductions, feature rows, and two fixtures with slow
modes: AR(1) torsions as feature rows (for `fit_tica`) and the dipeptide with its psi and phi driven by AR(1) processes (for the meter).

BOUNDS.  A sum of n exactly representable terms added in ANY order is within gamma_{n-1} sum |term| of the exact sum (Higham, Accuracy and
Stability of Numerical Algorithms, eq. 4.4), gamma_n = n u / (1 - n u), u = 2^-53.  The products of the moments are exact (fp32 x fp32 in
fp64), so N terms give gamma_N sum |a||b| with room to spare; the terms of the projection and of the autocovariance carry one rounding
each (a difference times a weight, a product of two doubles), which adds one to the index.  The expected values are computed by numpy in
another order, itself within the same bound of the exact sum: the tests allow twice the bound between the two.

AR(1) FIXTURES.  delta_k(t) = rho_k delta_k(t-1) + sqrt(1 - rho_k^2) sigma xi: a torsion fluctuating about its rest value with correlation
time -1 / log(rho_k).  Of its (cos, sin) pair one combination is linear in delta (lag-tau autocorrelation rho^tau) and one quadratic
(rho^(2 tau)), so K torsions give 2 K modes with well separated eigenvalues when the rho_k are spread: the eigenvalue gaps are asserted
where a fixture is made, because the eigenvectors of a near-degenerate pair are not a function of the moments that a tolerance can follow.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -53


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def feature_rows(T: int, W: int, seed: int = 0) -> np.ndarray:
    """float32 [T, W]: columns of different scales and offsets (cos / sin like values, distances, a large and a tiny column), no zeros."""
    rng = np.random.RandomState(seed + 1000 * W + T)
    scale = np.array([1.0, 0.5, 3.0, 1e-3, 40.0])[np.arange(W) % 5]
    offset = np.array([0.0, 0.3, -2.0, 0.0, 10.0])[np.arange(W) % 5]
    return _frozen((offset[None, :] + scale[None, :] * rng.randn(T, W)).astype(np.float32))


def moments_bounds(x: np.ndarray, lag: int):
    """(bound of sums [2, W], bound of moments [3, W, W]) for the fp32 rows ``x``: gamma_N sum |a||b| entry by entry."""
    a, b = np.abs(x[: x.shape[0] - lag].astype(np.float64)), np.abs(x[lag:].astype(np.float64))
    g = gamma(a.shape[0])
    return g * np.stack([a.sum(0), b.sum(0)]), g * np.stack([a.T @ a, b.T @ b, a.T @ b])


def projection_bound(x: np.ndarray, mean: np.ndarray, v: np.ndarray) -> np.ndarray:
    """[T, d]: gamma_{W+1} sum_j |x - mean||v|."""
    return gamma(x.shape[1] + 1) * (np.abs(x.astype(np.float64) - mean[None, :]) @ np.abs(v))


def autocov_bound(y: np.ndarray, max_lag: int) -> np.ndarray:
    """[max_lag + 1]: gamma_{T+1} sum_t |y_t y_{t+k}|."""
    T = y.shape[0]
    a = np.abs(y)
    return gamma(T + 1) * np.array([np.dot(a[: T - k], a[k:]) if k < T else 0.0 for k in range(max_lag + 1)])


def autocov_loop(y: np.ndarray, max_lag: int) -> np.ndarray:
    """An independent check, written for the tests: the adjusted autocovariance without the mean removed by a double loop (NaN for k >= T)."""
    T = len(y)
    out = np.full(max_lag + 1, np.nan)
    for k in range(min(max_lag + 1, T)):
        s = 0.0
        for t in range(T - k):
            s += float(y[t]) * float(y[t + k])
        out[k] = s / (T - k)
    return out


# ---- AR(1) torsions ----------------------------------------------------------------------------------------------------------------------------

def ar1(T: int, rhos, sigma: float, seed: int) -> np.ndarray:
    """float64 [T, K]: stationary AR(1) processes of standard deviation ``sigma`` and lag-1 correlations ``rhos``."""
    rng = np.random.RandomState(seed)
    rhos = np.asarray(rhos, dtype=np.float64)
    out = np.empty((T, rhos.shape[0]))
    out[0] = sigma * rng.randn(rhos.shape[0])
    kick = sigma * np.sqrt(1.0 - rhos * rhos)
    for t in range(1, T):
        out[t] = rhos * out[t - 1] + kick * rng.randn(rhos.shape[0])
    return out


FIT_RHOS, FIT_SIGMA, FIT_LAG, FIT_T = (0.985, 0.9, 0.6), 0.6, 5, 6000
MIN_GAP = 0.02  # lambda_0 - lambda_1 and lambda_1 - lambda_2 of a fixture, at least


def check_gaps(eigenvalues) -> None:
    lam = np.asarray(eigenvalues)
    assert lam.shape[0] >= 3 and lam[0] - lam[1] >= MIN_GAP and lam[1] - lam[2] >= MIN_GAP, lam.tolist()


@functools.lru_cache(maxsize=None)
def fit_fixture(seed: int = 3, T: int = FIT_T) -> np.ndarray:
    """float32 [T, 6]: interleaved (cos, sin) of three AR(1) torsions about rest values 0.4, -1.0 and 2.5 rad."""
    theta = np.array([0.4, -1.0, 2.5])[None, :] + ar1(T, FIT_RHOS, FIT_SIGMA, seed)
    return _frozen(np.stack([np.cos(theta), np.sin(theta)], axis=2).reshape(T, 6).astype(np.float32))


# ---- the dipeptide with driven torsions ----------------------------------------------------------------------------------------------------------

def _rotate(pos: np.ndarray, a: int, b: int, moving, angle: np.ndarray) -> np.ndarray:
    """``pos [T, n, 3]`` with the atoms ``moving`` turned by ``angle [T]`` about the axis from atom ``a`` to atom ``b`` (Rodrigues)."""
    axis = pos[:, b] - pos[:, a]
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    out = pos.copy()
    c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
    for m in moving:
        r = pos[:, m] - pos[:, b]
        out[:, m] = pos[:, b] + r * c + np.cross(axis, r) * s + axis * (axis * r).sum(1, keepdims=True) * (1.0 - c)
    return out


METER_RHOS, METER_SIGMA, METER_LAG, METER_ACF_LAG = (0.97, 0.8), 0.5, 5, 40


def dipeptide_torsion_frames(mol: dict, T: int, seed: int) -> np.ndarray:
    """float32 [T, 10, 3]: the Ala-Gly dipeptide (N CA CB C O | N CA C O OXT) with psi of ALA (about CA - C: atoms 4..9 turn) and phi of GLY
    (about N - CA: atoms 7..9 turn) following two AR(1) processes, every frame shifted as a whole, and 1e-3 nm of noise on every atom."""
    rng = np.random.RandomState(seed + 77)
    delta = ar1(T, METER_RHOS, METER_SIGMA, seed)
    pos = np.repeat(np.asarray(mol["pos"].numpy(), dtype=np.float64)[None], T, axis=0)
    pos = _rotate(pos, 1, 3, (4, 5, 6, 7, 8, 9), delta[:, 0])
    pos = _rotate(pos, 5, 6, (7, 8, 9), delta[:, 1])
    pos += 0.2 * rng.randn(T, 1, 3) + 1e-3 * rng.randn(T, pos.shape[1], 3)
    return _frozen(pos.astype(np.float32))


def torsion_batches(mol: dict, device, chains: int, T: int, n_batches: int, seed: int):
    """Samples as the callbacks receive them: per chain the ``[n, T, 3]`` view ``block[c]`` of a ``[chains, n, T, 3]`` block on ``device``
    (its ``transpose(0, 1)`` is `_frames_common.chain_view`'s layout), frames of `dipeptide_torsion_frames`, another seed for every chain."""
    out = []
    for b in range(n_batches):
        frames = [dipeptide_torsion_frames(mol, T, seed + 10 * b + c) for c in range(chains)]
        block = torch.from_numpy(np.stack([np.array(f.transpose(1, 0, 2), order="C") for f in frames])).to(device)
        out.append([{"dataset_label": "m", "atom_type_index": mol["atom_type_index"], "xhat_traj": block[c]} for c in range(chains)])
    return out


METER_REFERENCE_T, METER_CHAIN_T = 1500, 300


def perturbed(sums: np.ndarray, moments: np.ndarray, bound_s: np.ndarray, bound_m: np.ndarray, seed: int):
    """The moments moved by their full rounding bound with random signs (G and H kept symmetric, as both paths give them)."""
    rng = np.random.RandomState(seed)
    sign = lambda shape: np.where(rng.rand(*shape) < 0.5, -1.0, 1.0)
    W = sums.shape[1]
    sm = np.stack([np.triu(sign((W, W))) for _ in range(3)])
    sm[0] = sm[0] + np.triu(sm[0], 1).T
    sm[1] = sm[1] + np.triu(sm[1], 1).T
    sm[2] = sign((W, W))
    return sums + sign(sums.shape) * bound_s, moments + sm * bound_m


def meter_fixture(mol: dict, device):
    """(reference frames [METER_REFERENCE_T, 10, 3] as a CPU tensor, two batches of three chains of METER_CHAIN_T frames on ``device``)."""
    return torch.from_numpy(np.array(dipeptide_torsion_frames(mol, METER_REFERENCE_T, 500))), torsion_batches(mol, device, 3, METER_CHAIN_T, 2, seed=600)


def measure_meter_sensitivity(features_ref: np.ndarray, features_chains, draws: int = 16) -> dict:
    """How far the meter's outputs move when the reference moments move by their rounding bound: the moments of the fp32 feature rows
    ``features_ref`` are moved by `perturbed` (``draws`` draws of the signs), the model is refitted, and reference and chains
    (``features_chains``: a list of feature rows) are projected again.  Returns the largest absolute change of ``mean``, ``eigenvalues``,
    ``eigenvectors``, ``tic01`` (reference and chains), ``autocov`` (reference, chains, joined) and ``js_distance`` (every chain and the
    joined trajectory, one and two components) over the draws."""
    from jamun_amd import tica

    n_pairs = features_ref.shape[0] - METER_LAG
    sums, moments = tica.lagged_moments_host(features_ref, METER_LAG)
    bound_s, bound_m = moments_bounds(features_ref, METER_LAG)

    def outputs(s, m):
        fit = tica.fit_tica(s, m, n_pairs)
        check_gaps(fit["eigenvalues"])
        proj = [tica.project_host(f, fit["mean"], fit["eigenvectors"]) for f in [features_ref] + list(features_chains)]
        sums_k = [tica.autocov_sums_host(p[:, 0], METER_ACF_LAG) for p in proj]
        counts = [tica.autocov_counts(p.shape[0], METER_ACF_LAG) for p in proj]
        acf = [tica.autocov_from_sums(a, c) for a, c in zip(sums_k, counts)] + [tica.autocov_from_sums(np.sum(sums_k[1:], 0), np.sum(counts[1:], 0))]
        trajs = [p[:, :2] for p in proj[1:]] + [np.concatenate([p[:, :2] for p in proj[1:]])]
        js = [v for t in trajs for v in tica.tica_js_distances(t, proj[0][:, :2], 100, 50).values()]
        return {"mean": fit["mean"], "eigenvalues": fit["eigenvalues"], "eigenvectors": fit["eigenvectors"],
                "tic01": np.concatenate([p[:, :2] for p in proj]), "autocov": np.concatenate(acf), "js_distance": np.array(js)}

    base = outputs(sums, moments)
    worst = {k: 0.0 for k in base}
    for seed in range(draws):
        moved = outputs(*perturbed(sums, moments, bound_s, bound_m, seed))
        for k in base:
            worst[k] = max(worst[k], float(np.max(np.abs(moved[k] - base[k]))))
    return worst


# The meter's device path against its host path on the fixture above (test_gpu_tica.py): the tolerance of each output is TEN TIMES the
# largest change `measure_meter_sensitivity` observed on this fixture with 16 draws (absolute values; the eigenvectors are of order 1, the
# projections of order 1, the autocovariance of order 0.1 to 1).  test_tica_host.py repeats the measurement and checks that the constants
# below are what it finds (within a factor 2), so they cannot drift from the fixture.  The JS distances did not change in any draw (no
# projected value lies within 1e-11 of a bin edge: the counts are the same integers), so ten times the observed change is 0 and the
# distances of the two paths are compared for equality.
METER_OBSERVED = {"mean": 1.45e-13, "eigenvalues": 1.33e-11, "eigenvectors": 6.77e-11, "tic01": 7.38e-11, "autocov": 9.17e-12, "js_distance": 0.0}
METER_TOLERANCE = {k: 10.0 * v for k, v in METER_OBSERVED.items()}
