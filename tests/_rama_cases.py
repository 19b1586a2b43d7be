"""Cases for the Ramachandran tests (test_rama_host.py, test_gpu_rama.py): seeded, no GPU.

ANGLES.  `special_values(bins)` is where a binning rule can go wrong: every edge of ``np.linspace(-pi, pi, bins + 1)`` cast to float32 and
the next float32 either side of it, +-float32(pi) (which lie OUTSIDE [-pi, pi] in float64), -0.0 and 0.0, and the non-finite values NaN
and +-inf.  `angle_table(T, W, bins)` fills a float32 ``[T, W]`` array with them (every column a different rotation of the list, so that a
pair of columns meets finite-finite, finite-NaN and NaN-NaN frames) followed by uniform draws.

`numpy_rule(x, y, bins)` is the pinned rule: ``np.histogram2d`` of the clipped float64 values of the frames whose x and y are finite.

MOLECULES.  The Ala-Gly dipeptide of the trajectory tests, and `synth.peptide` for the tripeptide and the five-residue chain.
"""
import functools

import numpy as np

BINS = (1, 2, 7, 100, 128)
F32_PI = np.float32(np.pi)


def special_values(bins: int) -> np.ndarray:
    """float32 [K]: see the module docstring.  The finite ones first, then NaN, +inf, -inf."""
    e = np.linspace(-np.pi, np.pi, bins + 1).astype(np.float32)
    below, above = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
    finite = np.concatenate([e, below, above, [F32_PI, -F32_PI, np.float32(-0.0), np.float32(0.0)]]).astype(np.float32)
    finite = finite[np.abs(finite) <= np.nextafter(F32_PI, np.float32(np.inf))]  # (nothing an atan2f could not return, give or take a step)
    return np.concatenate([finite, np.array([np.nan, np.inf, -np.inf], dtype=np.float32)])


@functools.lru_cache(maxsize=None)
def angle_table(T: int, W: int, bins: int, seed: int = 0) -> np.ndarray:
    """float32 [T, W]: the special values of ``bins`` (column w rotated by 7 w + 1 places), then uniform draws in [-pi, pi)."""
    rng = np.random.RandomState(1000 * bins + 10 * W + seed)
    s = special_values(bins)
    out = rng.uniform(-np.pi, np.pi, size=(T, W)).astype(np.float32)
    k = min(T, len(s))
    for w in range(W):
        out[:k, w] = np.roll(s, 7 * w + 1)[:k]
    out.setflags(write=False)
    return out


def numpy_rule(x: np.ndarray, y: np.ndarray, bins: int) -> np.ndarray:
    """What the issue pins the rule to: np.histogram2d of the clipped float64 angles of the finite frames, as integers [bins, bins]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    h, _, _ = np.histogram2d(np.clip(x[ok], -np.pi, np.pi), np.clip(y[ok], -np.pi, np.pi), bins, range=((-np.pi, np.pi), (-np.pi, np.pi)))
    assert (h == np.round(h)).all()
    return h.astype(np.int64)


def cut_sets(T: int) -> list:
    """Cuts for ``T`` frames: one segment; the first frame alone; cuts on and off 64-frame boundaries; 64 cuts (or T of them)."""
    sets = [[T]]
    if T > 1:
        sets.append([1, T])
    if T > 64:
        sets.append(sorted(v for v in {63, 64, 65, 128, T - 1, T} if v <= T))
    many = np.unique(np.linspace(1, T, 64).astype(np.int64)).tolist()
    if many not in sets:
        sets.append(many)
    return sets


@functools.lru_cache(maxsize=None)
def molecules() -> dict:
    from _traj_molecules import dipeptide
    from jamun_amd import synth

    return {"AG": dipeptide(), "tri": synth.peptide("AGS", seed=3), "penta": synth.peptide("AGSKW", seed=5)}


def random_counts(C: int, P: int, B: int, seed: int, density: float = 0.3) -> np.ndarray:
    """uint32 [C, P, B, B] segment counts with empty bins (a share ``1 - density`` of them) and counts up to 1000."""
    rng = np.random.RandomState(seed)
    return (rng.randint(1, 1000, size=(C, P, B, B)) * (rng.uniform(size=(C, P, B, B)) < density)).astype(np.uint32)


def chain_frames(sample) -> np.ndarray:
    """A sample's ``xhat_traj [n, T, 3]`` as float32 frames [T, n, 3] on the host."""
    return np.ascontiguousarray(sample["xhat_traj"].permute(1, 0, 2).cpu().numpy())
