"""GPU tests of jamun_hist.hip (k_hist2d_pairs, k_js_divergence) and of the Ramachandran meter on the device path.  The expected values
are the host specification's (jamun_amd/ramachandran.py, itself pinned to np.histogram2d and scipy in test_rama_host.py): counts integer
for integer on the same float32 angles, divergences within JSD_TOL."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _rama_cases as rc
from _intcoord_cases import TORSION_TOL_RAD, _well_conditioned, tumbling_batches
from _frames_common import CaseDataset, StubSampler, _dev, guarded, intact, run, tree
from _traj_molecules import dipeptide
from jamun_amd import ramachandran as R

pytestmark = pytest.mark.gpu

# k_js_divergence against js_divergence_host on identical counts.  The sum of |terms| is at most 2 ln 2; a few ulp of fp64 log per term
# and a tree sum over at most 1.6e4 bins put the error near 3e-15; 1e-12 leaves a factor of 300, and is seven orders below what moving
# one sample of 1e5 does.
JSD_TOL = 1e-12
SENTINEL = -77
SLICE = 4096  # JAMUN_HIST_SLICE (test_rama_host.py checks that native.HIST_SLICE mirrors the header)


def _padded(a: np.ndarray, dev, pad: int = 3) -> torch.Tensor:
    """``a [T, W]`` on the device as a view of a [T, W + pad] array of NaN: the row stride is not the width."""
    T, W = a.shape
    big = torch.full((T, W + pad), float("nan"), dtype=torch.float32, device=dev)
    big[:, :W] = torch.from_numpy(np.array(a)).to(dev)
    view = big[:, :W]
    assert T == 1 or view.stride(0) == W + pad
    return view


def _pairs(W: int, P: int) -> np.ndarray:
    """P pairs over W columns; with P > 1 a pair of one column with itself and a pair given twice."""
    rows = [[0, W - 1], [W - 1, W - 1], [0, W - 1]] + [[(3 * k) % W, (5 * k + 1) % W] for k in range(P)]
    return np.array(rows[:P], dtype=np.int32)


@pytest.mark.parametrize("bins", rc.BINS)
def test_counts_equal_the_host_specification_integer_for_integer(bins):
    """Frame counts around a wave and around a slice of a segment; one cut, the first frame alone, cuts on and off 64-frame boundaries, 64
    cuts; 1 and 9 pairs with a repeated column; 2, 3 and 7 columns in rows of a longer stride; angles on every edge, one float32 either
    side of it, +-float32(pi), -0.0, NaN and +-inf."""
    from jamun_amd import native

    dev = _dev()
    assert native.HIST_SLICE == SLICE
    for T in (1, 63, 64, 65, SLICE, SLICE + 1):
        for W, P in ((2, 1), (3, 9), (7, 9)):
            a = rc.angle_table(SLICE + 1, W, bins)[:T]
            x = _padded(a, dev)
            pairs = _pairs(W, P)
            for cuts in rc.cut_sets(T):
                want, want_skipped = R.histogram_host(a, pairs, bins, cuts)
                big, out = guarded((len(cuts), P, bins, bins), dev, torch.int32, SENTINEL)
                big_s, sk = guarded((len(cuts), P), dev, torch.int32, SENTINEL)
                got, got_skipped = native.hist2d_pairs(x, pairs, bins, cuts, out=out, skipped=sk)
                torch.cuda.synchronize()
                what = (T, W, P, cuts[:4])
                assert got.data_ptr() == out.data_ptr() and intact(big, SENTINEL) and intact(big_s, SENTINEL), what
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want), what
                assert np.array_equal(got_skipped.cpu().numpy().astype(np.int64), want_skipped), what
    assert want_skipped.sum() > 0 and want.sum() > 0


def test_4096_frames_in_one_bin():
    from jamun_amd import native

    dev = _dev()
    a = np.full((4096, 2), 1.0, dtype=np.float32)
    a[:, 1] = -2.0
    want, _ = R.histogram_host(a, [[0, 1]], 100, [4096])
    got, skipped = native.hist2d_pairs(torch.from_numpy(a).to(dev), [[0, 1]], 100, [4096])
    assert int(want.max()) == 4096 and np.array_equal(got.cpu().numpy().view(np.uint32), want) and int(skipped.sum()) == 0


def test_a_device_resident_pair_table_with_a_column_out_of_range_counts_nothing_for_that_pair():
    from jamun_amd import native

    dev = _dev()
    W, bins, T = 3, 7, 200
    a = rc.angle_table(T, W, bins)
    table = np.array([[0, 1], [0, W], [-1, 0], [2, 0], [2 ** 31 - 1, 1]], dtype=np.int32)
    good = [0, 3]
    want, want_skipped = R.histogram_host(a, table[good], bins, [64, T])
    got, skipped = native.hist2d_pairs(_padded(a, dev), torch.from_numpy(table).to(dev), bins, [64, T])
    got, skipped = got.cpu().numpy().view(np.uint32), skipped.cpu().numpy()
    assert np.array_equal(got[:, good], want) and np.array_equal(skipped[:, good], want_skipped)
    assert not got[:, [1, 2, 4]].any() and not skipped[:, [1, 2, 4]].any()
    with pytest.raises(ValueError, match="pairs table on the device"):
        native.hist2d_pairs(_padded(a, dev), torch.from_numpy(table).to(dev).long(), bins, [T])


def test_the_c_entries_refuse_bad_arguments_and_write_nothing():
    from jamun_amd import _lib

    dev = _dev()
    lib = _lib.load()
    T, W, bins = 100, 2, 4
    a = torch.zeros(T, W, device=dev)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    edges = torch.from_numpy(np.linspace(-np.pi, np.pi, bins + 1)).to(dev)
    big, out = guarded((2, 1, bins, bins), dev, torch.int32, SENTINEL)
    big_s, sk = guarded((2, 1), dev, torch.int32, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream

    def call(cuts, capacity=None, b=bins, stride=W):
        c = np.asarray(cuts, dtype=np.int32)
        return lib.jamun_hist2d_pairs(a.data_ptr(), stride, T, W, pairs.data_ptr(), 1, edges.data_ptr(), b, c.ctypes.data, len(c), out.data_ptr(),
                                      out.numel() if capacity is None else capacity, sk.data_ptr(), st)

    assert call([50, 100], capacity=2 * bins * bins - 1) == -1 and b"counts_capacity" in lib.jamun_last_error()
    for bad in ([0, 50], [50, 50], [60, 50], [50, 101]):
        assert call(bad) == -1 and b"cuts" in lib.jamun_last_error()
    assert call([50, 100], b=0) == -1 and call([50, 100], b=129) == -1 and b"bins" in lib.jamun_last_error()
    assert call([50, 100], stride=1) == -1 and b"row_stride" in lib.jamun_last_error()
    assert call(list(range(1, 66))) == -1 and b"n_cuts" in lib.jamun_last_error()
    torch.cuda.synchronize()
    assert (big == SENTINEL).all() and (big_s == SENTINEL).all()
    assert call([50, 100]) == 0
    torch.cuda.synchronize()
    assert intact(big, SENTINEL) and out.sum().item() == 100
    pooled = torch.zeros(2, dtype=torch.float64, device=dev)
    per_pair = torch.zeros(2, 1, dtype=torch.float64, device=dev)
    js = lambda n_ref, b=bins: lib.jamun_js_divergence(out.data_ptr(), 2, 1, b, out.data_ptr(), n_ref, pooled.data_ptr(), per_pair.data_ptr(), st)
    assert js(2) == -1 and b"n_ref_pairs" in lib.jamun_last_error()
    assert js(1, 129) == -1 and b"bins" in lib.jamun_last_error()
    assert js(1) == 0
    torch.cuda.synchronize()


# ---- the divergence ---------------------------------------------------------------------------------------------------------------------

def _as_dev(counts: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).to(dev)


@pytest.mark.parametrize("B, P, C", [(1, 1, 1), (2, 3, 5), (7, 2, 64), (100, 1, 11), (128, 9, 3)])
def test_js_divergence_matches_the_host_specification(B, P, C):
    from jamun_amd import native

    dev = _dev()
    counts = rc.random_counts(C, P, B, seed=B + C)
    ref = rc.random_counts(1, P, B, seed=B + 1, density=0.5)[0] + (np.arange(B * B).reshape(B, B) == 0).astype(np.uint32)
    worst = 0.0
    for r in (ref, ref[0]):  # a reference per pair, and one for all
        want = R.js_divergence_host(counts, r)
        pooled, per_pair = native.js_divergence(_as_dev(counts, dev), _as_dev(r, dev))
        again = native.js_divergence(_as_dev(counts, dev), _as_dev(r, dev))
        assert pooled.dtype == torch.float64 and tuple(pooled.shape) == (C,) and tuple(per_pair.shape) == (C, P)
        assert torch.equal(pooled.view(torch.int64), again[0].view(torch.int64)) and torch.equal(per_pair.view(torch.int64), again[1].view(torch.int64))
        for got, exp in ((pooled.cpu().numpy(), want["pooled"]), (per_pair.cpu().numpy(), want["per_pair"])):
            assert np.array_equal(np.isnan(got), np.isnan(exp))
            ok = ~np.isnan(exp)
            if ok.any():
                worst = max(worst, float(np.abs(got[ok] - exp[ok]).max()))
    print(f"B={B} P={P} C={C}: k_js_divergence vs host: {worst:.2e} (bound {JSD_TOL:g})")
    assert worst <= JSD_TOL


def test_js_divergence_at_its_ends():
    from jamun_amd import native

    dev = _dev()
    B = 100
    counts = rc.random_counts(2, 2, B, seed=3)
    pooled, per_pair = native.js_divergence(_as_dev(counts[:1], dev), _as_dev(counts[0], dev))
    assert pooled.cpu().tolist() == [0.0] and per_pair.cpu().tolist() == [[0.0, 0.0]]  # identical histograms: exactly zero
    left, right = np.zeros((2, 1, B, B), dtype=np.uint32), np.zeros((B, B), dtype=np.uint32)
    left[1, 0, :3] = 5   # the first segment is empty: NaN for the first cut
    right[3:] = 2
    pooled, per_pair = native.js_divergence(_as_dev(left, dev), _as_dev(right, dev))
    assert math.isnan(pooled[0].item()) and math.isnan(per_pair[0, 0].item())
    assert abs(pooled[1].item() - math.log(2.0)) <= JSD_TOL and abs(per_pair[1, 0].item() - math.log(2.0)) <= JSD_TOL
    big = np.zeros((1, 1, 2, 2), dtype=np.uint32)
    big[0, 0, 0, 0], big[0, 0, 1, 1] = 3_000_000_000, 1  # a counter above 2^31 is read as unsigned
    pooled, _ = native.js_divergence(_as_dev(big, dev), _as_dev(np.array([[1, 0], [0, 1]], dtype=np.uint32), dev))
    assert abs(pooled[0].item() - R.js_divergence_host(big, np.array([[1, 0], [0, 1]]))["pooled"][0]) <= JSD_TOL


# ---- the meter on the device path ---------------------------------------------------------------------------------------------------------

SIGMA = 0.01  # nm of noise on every coordinate of the tumbling dipeptide: every frame stays well conditioned (the premise of TORSION_TOL_RAD)


def _entropy2(e: float) -> float:
    return 0.0 if e <= 0.0 or e >= 1.0 else -(e * math.log(e) + (1.0 - e) * math.log(1.0 - e))


def _jsd_moved(k: int, n: int, bins_total: int) -> float:
    """How far JSD(p, q) can move when k of the n samples behind p change their bin.  p = (1 - e) r + e v becomes (1 - e) r + e u with
    e = k / n and distributions r, u, v; for a mixture (1 - e) H(r) + e H(v) <= H(p) <= (1 - e) H(r) + e H(v) + h(e), so H(p) moves by at
    most e ln K + h(e) and H((p + q) / 2), where the moved weight is e / 2, by (e / 2) ln K + h(e / 2).  JSD = H(m) - H(p) / 2 - H(q) / 2."""
    if k == 0:
        return 0.0
    e = min(1.0, k / n)
    return e * math.log(bins_total) + _entropy2(e / 2) + _entropy2(e) / 2


def _near_edge(frames: np.ndarray, index: np.ndarray, bins: int) -> np.ndarray:
    """Per frame: does its fp64 phi or psi lie within TORSION_TOL_RAD of a bin edge (the first and last edge included)?"""
    from jamun_amd.features import internal_coords_host

    a = internal_coords_host(frames, index)
    e = np.linspace(-np.pi, np.pi, bins + 1)
    return (np.abs(a[:, :, None] - e[None, None, :]).min(axis=2) <= TORSION_TOL_RAD).any(axis=1)


def test_meter_on_device_tensors_writes_the_host_paths_files_except_at_bin_edges(tmp_path):
    """4 chains x 300 frames of the tumbling Ala-Gly dipeptide with SIGMA of noise, two batches, and 500 further frames as the reference
    trajectory.  The device path (float32 torsions from the kernel) and device="host" (fp64 torsions rounded to float32) may put a frame in
    different bins only if its fp64 phi or psi lies within TORSION_TOL_RAD of an edge: each such frame moves at most one count, L1 <= 2."""
    from jamun_amd.callbacks import RamachandranMetricsCallback

    dev = _dev()
    mol = dipeptide()
    chains, T, bins = 4, 300, 100
    batches = tumbling_batches(mol, dev, chains, T, 2, seed=21, sigma=SIGMA)
    reference = rc.chain_frames(tumbling_batches(mol, torch.device("cpu"), 1, 500, 1, seed=22, sigma=SIGMA)[0][0])
    index, pairs, _ = R.phi_psi_pairs(mol)
    frames = [rc.chain_frames(s) for b in batches for s in b]
    for fr in frames + [reference]:
        assert _well_conditioned(fr.astype(np.float64), index).all()
    near = [_near_edge(fr, index, bins) for fr in frames]
    near_ref = int(_near_edge(reference, index, bins).sum())
    n_near = sum(int(m.sum()) for m in near)
    print(f"frames within {TORSION_TOL_RAD:g} rad of a bin edge: {n_near} of {2 * chains * T} samples, {near_ref} of {len(reference)} reference frames")
    assert n_near <= 0.01 * 2 * chains * T and near_ref <= 0.01 * len(reference)

    ds = CaseDataset(mol, "m")
    runs = {}
    for mode in ("device", "host"):
        cb = RamachandranMetricsCallback([ds], output_dir=str(tmp_path / mode), bins=bins, reference=reference, device=mode)
        smp = StubSampler(dev)
        run(cb, batches, smp)
        runs[mode] = (cb, smp, tmp_path / mode / "m" / "ramachandran")
    d, h = runs["device"][2], runs["host"][2]
    assert sorted(os.listdir(d)) == sorted(os.listdir(h)) == sorted([f"{i}.npz" for i in range(2 * chains)] + ["joined.npz", "pairs.json", "true_traj.npz"])
    assert open(d / "pairs.json", "rb").read() == open(h / "pairs.json", "rb").read()
    ref_d, ref_h = np.load(d / "true_traj.npz")["counts"], np.load(h / "true_traj.npz")["counts"]
    assert ref_d.dtype == np.uint32 and ref_d.sum() == ref_h.sum() == len(reference)
    assert np.abs(ref_d.astype(np.int64) - ref_h.astype(np.int64)).sum() <= 2 * near_ref
    K = bins * bins
    worst = 0.0
    for name in [str(i) for i in range(2 * chains)] + ["joined"]:
        zd, zh = np.load(d / f"{name}.npz"), np.load(h / f"{name}.npz")
        assert sorted(zd.files) == sorted(zh.files) == ["counts", "js_divergence", "js_divergence_per_pair", "num_samples", "skipped"]
        m = np.concatenate(near) if name == "joined" else near[int(name)]
        assert zd["counts"].dtype == np.uint32 and zd["counts"].shape == (1, bins, bins) and zd["counts"].sum() == len(m)
        assert np.abs(zd["counts"].astype(np.int64) - zh["counts"].astype(np.int64)).sum() <= 2 * int(m.sum())
        assert np.array_equal(zd["num_samples"], zh["num_samples"]) and zd["num_samples"].tolist() == R.sample_counts(len(m))
        assert np.array_equal(zd["skipped"], zh["skipped"]) and not zd["skipped"].any()
        for c, k in enumerate(zd["num_samples"].tolist()):
            bound = _jsd_moved(int(m[:k].sum()), k, K) + _jsd_moved(near_ref, len(reference), K) + JSD_TOL
            for key in ("js_divergence", "js_divergence_per_pair"):
                dev_h = float(np.abs(zd[key][c] - zh[key][c]).max())
                worst = max(worst, dev_h)
                assert dev_h <= bound, (name, k, key, dev_h, bound)
    print(f"device vs host JSD files: {worst:.2e}")
    logged_d, logged_h = runs["device"][1].fabric.logged, runs["host"][1].fabric.logged
    assert len(logged_d) == len(logged_h) == 2 and list(logged_d[1]) == ["m/js_divergence/pred_traj_joined"]
    assert logged_d[1]["m/js_divergence/pred_traj_joined"] == float(np.load(d / "joined.npz")["js_divergence"][-1])
    # the device path kept its tables on the device and the host path never touched it
    assert runs["device"][0].meters["m"]._dev and not runs["host"][0].meters["m"]._dev


def test_metric_files_are_the_same_bytes_with_superposed_trajectory_files(tmp_path):
    """The histograms come from the RAW frames: beside a SaveTrajectoryCallback that superposes the frames it writes (on the device, from
    the same sample tensors) the metric files are byte for byte those beside one that does not."""
    from jamun_amd.callbacks import RamachandranMetricsCallback, SaveTrajectoryCallback

    dev = _dev()
    mol = dipeptide()
    batches = tumbling_batches(mol, dev, 2, 150, 2, seed=23, sigma=SIGMA)
    reference = rc.chain_frames(batches[0][0])
    ds = CaseDataset(mol, "m")
    trees = {}
    for superpose in (False, True):
        root = tmp_path / ("on" if superpose else "off")
        save = SaveTrajectoryCallback([ds], output_dir=str(root), encode="device", superpose=superpose)
        meter = RamachandranMetricsCallback([ds], output_dir=str(root), bins=50, reference=reference)
        smp = StubSampler(dev)
        for cb in (save, meter):
            cb.on_sample_start(smp)
        for b in batches:
            for cb in (save, meter):
                cb.on_after_sample_batch(b, smp)
            save.flush()
        for cb in (save, meter):
            cb.on_sample_end(smp)
        files = tree(str(root))
        trees[superpose] = {f: v for f, v in files.items() if os.sep + "ramachandran" + os.sep in f}
        assert any("rmsd" in f for f in files) == superpose
    assert len(trees[True]) == 4 + 1 + 2 and trees[True] == trees[False]
    z = np.load(tmp_path / "on" / "m" / "ramachandran" / "0.npz")
    assert z["js_divergence"][-1] == 0.0  # chain 0 is the reference
