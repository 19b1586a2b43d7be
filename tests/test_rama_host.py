"""Host tests of jamun_amd/ramachandran.py: the specification (sample counts, pairings, the binning rule pinned to np.histogram2d, the
JS divergence pinned to scipy), the argument checks of the device bindings that need no GPU, and the meter on CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

import _rama_cases as rc
from _intcoord_cases import tumbling_batches
from _frames_common import CaseDataset, StubSampler, meter_run, run, tree
from jamun_amd import ramachandran as R


def test_sample_counts_are_the_references_sequence():
    doubling = [100, 200, 400, 800, 1600, 3200, 6400, 12800, 25600, 51200]
    assert R.sample_counts(50) == [50]
    assert R.sample_counts(100) == [100]
    assert R.sample_counts(101) == [100, 101]
    assert R.sample_counts(20000) == doubling[:8] + [20000]
    assert R.sample_counts(51201) == doubling + [51201]
    assert R.sample_counts(10 ** 6) == doubling + [10 ** 6]


def _residue_of(label: str) -> int:
    return int(label.split()[3])


@pytest.mark.parametrize("name, n_res", [("AG", 2), ("tri", 3), ("penta", 5)])
def test_both_pairings(name, n_res):
    mol = rc.molecules()[name]
    index, pairs, labels = R.phi_psi_pairs(mol)
    assert index.dtype == np.int32 and index.shape == (2 * (n_res - 1), 4) and pairs.dtype == np.int32
    assert pairs.tolist() == [[i, n_res - 1 + i] for i in range(n_res - 1)] and len(labels) == n_res - 1
    names = list(mol["atom_names"])
    for a, b in pairs.tolist():  # phi = C N CA C, psi = N CA C N, and the reference's pair is phi of residue i + 1 with psi of residue i
        assert [names[v] for v in index[a]] == ["C", "N", "CA", "C"] and [names[v] for v in index[b]] == ["N", "CA", "C", "N"]
        assert index[a, 0] == index[b, 2] and index[a, 1] == index[b, 3]
    for l in labels:
        phi, psi = l.split(" / ")
        assert phi.startswith("PHI ") and psi.startswith("PSI ") and _residue_of(phi) == _residue_of(psi) + 1
    index_r, pairs_r, labels_r = R.phi_psi_pairs(mol, "residue")
    assert np.array_equal(index_r, index) and pairs_r.shape == (n_res - 2, 2) and len(labels_r) == n_res - 2
    for a, b in pairs_r.tolist():
        assert index[a, 1:].tolist() == index[b, :3].tolist()
    for l in labels_r:
        phi, psi = l.split(" / ")
        assert _residue_of(phi) == _residue_of(psi)


def test_the_dipeptide_has_one_reference_pair_and_no_residue_pair():
    mol = rc.molecules()["AG"]
    assert R.phi_psi_pairs(mol)[1].tolist() == [[0, 1]]
    assert R.phi_psi_pairs(mol, "residue")[1].shape == (0, 2)
    with pytest.raises(ValueError, match="pairing"):
        R.phi_psi_pairs(mol, "nearest")


def test_unequal_phi_and_psi_counts_are_refused_with_both_counts():
    mol = dict(rc.molecules()["tri"])
    names = list(mol["atom_names"])
    last_c = max(i for i, a in enumerate(names) if a == "C")
    names[last_c] = "CX"  # the last residue loses its C and with it its phi; the psi of residues 0 and 1 stay
    mol["atom_names"] = names
    with pytest.raises(ValueError, match="1 phi and 2 psi"):
        R.phi_psi_pairs(mol)
    assert R.phi_psi_pairs(mol, "residue")[1].tolist() == [[0, 2]]  # phi and psi of residue 1


@pytest.mark.parametrize("bins", rc.BINS)
def test_histogram_host_is_numpys_rule_after_the_clip(bins):
    T, W = 1200, 3
    a = rc.angle_table(T, W, bins)
    s = rc.special_values(bins)
    assert np.isnan(a).any() and np.isinf(a).any() and (a == rc.F32_PI).any() and (a == -rc.F32_PI).any() and T > len(s) or bins == 128
    pairs = np.array([[0, 1], [2, 0], [1, 1]], dtype=np.int32)
    counts, skipped = R.histogram_host(a, pairs, bins, [T])
    assert counts.dtype == np.uint32 and counts.shape == (1, 3, bins, bins) and skipped.dtype == np.int64 and skipped.shape == (1, 3)
    for p, (cx, cy) in enumerate(pairs.tolist()):
        want = rc.numpy_rule(a[:, cx], a[:, cy], bins)
        assert np.array_equal(counts[0, p].astype(np.int64), want)
        assert int(counts[0, p].sum()) + int(skipped[0, p]) == T and skipped[0, p] == int((~(np.isfinite(a[:, cx]) & np.isfinite(a[:, cy]))).sum())
    assert skipped.min() > 0
    for cuts in rc.cut_sets(T):
        c, s_ = R.histogram_host(a, pairs, bins, cuts)
        assert c.shape[0] == len(cuts)
        keep = cuts[-1]
        whole, sk = R.histogram_host(a[:keep], pairs, bins, [keep])
        assert np.array_equal(c.sum(axis=0, dtype=np.int64), whole[0]) and np.array_equal(s_.sum(axis=0), sk[0])
        lens = np.diff([0] + list(cuts))
        assert np.array_equal(c.reshape(len(cuts), 3, -1).sum(axis=2) + s_, np.repeat(lens[:, None], 3, axis=1))


def test_a_dihedral_of_exactly_180_degrees_is_kept_by_the_clip():
    a = np.array([[rc.F32_PI, 0.0], [-rc.F32_PI, 0.0], [3.0, 0.0]], dtype=np.float32)
    raw, _, _ = np.histogram2d(a[:, 0].astype(np.float64), a[:, 1].astype(np.float64), 100, range=((-np.pi, np.pi), (-np.pi, np.pi)))
    assert raw.sum() == 1  # numpy alone drops the two
    counts, skipped = R.histogram_host(a, [[0, 1]], 100, [3])
    assert counts.sum() == 3 and skipped.sum() == 0  # 1 of 3 counted raw, 3 of 3 after the clip
    # (linspace's middle edge of 100 bins is 4.4e-16, not 0: an angle of 0.0 lies in bin 49, as numpy puts it)
    assert counts[0, 0, 99, 49] == 1 and counts[0, 0, 0, 49] == 1 and counts[0, 0, 97, 49] == 1


def test_histogram_host_refuses_bad_arguments():
    a = np.zeros((10, 2), dtype=np.float32)
    for cuts in ([], [0, 5], [5, 5], [6, 5], [11], list(range(1, 66)), [[5]], [2.5]):
        with pytest.raises(ValueError, match="cuts"):
            R.histogram_host(np.zeros((100, 2), dtype=np.float32) if len(cuts) > 60 else a, [[0, 1]], 4, cuts)
    for pairs in ([[0, 2]], [[-1, 0]], [0, 1], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="pairs"):
            R.histogram_host(a, pairs, 4, [10])
    for bins in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="bins"):
            R.histogram_host(a, [[0, 1]], bins, [10])
    counts, skipped = R.histogram_host(a, np.zeros((0, 2), dtype=np.int32), 4, [10])
    assert counts.shape == (1, 0, 4, 4) and skipped.shape == (1, 0)


@pytest.mark.parametrize("B, P", [(1, 1), (2, 3), (7, 2), (100, 1), (128, 2)])
def test_js_divergence_host_is_scipys(B, P):
    from scipy.spatial.distance import jensenshannon

    C = 5
    counts = rc.random_counts(C, P, B, seed=B)
    counts[0, :, 0, 0] += 1  # (no prefix is empty: scipy has no answer there)
    ref = rc.random_counts(1, P, B, seed=B + 1, density=0.5)[0] + (np.arange(B * B).reshape(B, B) == 0)  # (never empty)
    got = R.js_divergence_host(counts, ref)
    assert got["pooled"].shape == (C,) and got["per_pair"].shape == (C, P) and got["pooled"].dtype == np.float64
    prefix = np.cumsum(counts.astype(np.int64), axis=0)
    for c in range(C):
        want = jensenshannon(prefix[c].sum(axis=0).ravel(), ref.sum(axis=0).ravel()) ** 2
        assert abs(got["pooled"][c] - want) <= 1e-14
        for p in range(P):
            assert abs(got["per_pair"][c, p] - jensenshannon(prefix[c, p].ravel(), ref[p].ravel()) ** 2) <= 1e-14
    one = R.js_divergence_host(counts, ref[0])  # one reference [B, B] for every pair
    for p in range(P):
        assert abs(one["per_pair"][C - 1, p] - jensenshannon(prefix[C - 1, p].ravel(), ref[0].ravel()) ** 2) <= 1e-14
    assert abs(one["pooled"][C - 1] - jensenshannon(prefix[C - 1].sum(axis=0).ravel(), ref[0].ravel()) ** 2) <= 1e-14


def test_js_divergence_host_at_its_ends():
    B = 7
    counts = rc.random_counts(3, 2, B, seed=1)
    same = R.js_divergence_host(counts[:1], counts[0])
    assert same["pooled"][0] == 0.0 and (same["per_pair"][0] == 0.0).all()
    assert R.js_divergence_host(counts[:1], 2 * counts[0])["pooled"][0] == 0.0  # (normalised: the scale does not matter)
    left, right = np.zeros((1, 1, B, B), dtype=np.uint32), np.zeros((B, B), dtype=np.uint32)
    left[0, 0, :3] = 5
    right[3:] = 2
    d = R.js_divergence_host(left, right)
    assert abs(d["pooled"][0] - np.log(2.0)) <= 1e-15 and abs(d["per_pair"][0, 0] - np.log(2.0)) <= 1e-15
    empty_first = np.concatenate([np.zeros_like(left), left])
    d = R.js_divergence_host(empty_first, right)
    assert np.isnan(d["pooled"][0]) and np.isnan(d["per_pair"][0, 0]) and abs(d["pooled"][1] - np.log(2.0)) <= 1e-15
    with pytest.raises(ValueError, match="no count"):
        R.js_divergence_host(left, np.zeros((B, B), dtype=np.uint32))
    with pytest.raises(ValueError, match="shape"):
        R.js_divergence_host(left, np.zeros((2, B, B), dtype=np.uint32))


def test_native_hist2d_pairs_checks_its_arguments_before_it_needs_a_gpu():
    from jamun_amd import native

    a = torch.zeros(100, 3)
    good = dict(pairs=[[0, 1]], bins=100, cuts=[100])

    def call(**over):
        return native.hist2d_pairs(a, **dict(good, **over))

    for pairs in ([[0, 3]], [[-1, 0]], [0, 1], [[0, 1, 2]], [[0.5, 1.0]], torch.zeros(2, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="pairs"):
            call(pairs=pairs)
    for bins in (0, 129, -3, 10.0, "100", True):
        with pytest.raises(ValueError, match="bins"):
            call(bins=bins)
    for cuts in ([], [0], [0, 50], [50, 50], [60, 50], [101], list(range(1, 66)), [[50]], [1.5]):
        with pytest.raises(ValueError, match="cuts"):
            call(cuts=cuts)
    with pytest.raises(ValueError, match="angles"):
        native.hist2d_pairs(torch.zeros(100), **good)
    with pytest.raises(RuntimeError, match="on the GPU"):  # everything above passed: only now a device is asked for
        call()
    assert native.HIST_MAX_BINS == 128 and native.HIST_MAX_CUTS == R.MAX_CUTS == 64
    assert np.array_equal(native.hist_edges(100), np.linspace(-np.pi, np.pi, 101))


def test_native_constants_mirror_the_header():
    import re

    from jamun_amd import native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "jamun_amd", "csrc", "jamun_internal.h")).read()
    value = lambda name: int(re.search(rf"#define {name}\s+(\d+)", h).group(1))
    assert value("JAMUN_HIST_SLICE") == native.HIST_SLICE and value("JAMUN_HIST_MAX_BINS") == native.HIST_MAX_BINS
    assert value("JAMUN_HIST_MAX_CUTS") == native.HIST_MAX_CUTS
    assert "jamun_hist.hip" in __import__("jamun_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


# ---- the meter on CPU tensors -----------------------------------------------------------------------------------------------------------

def _meter_run(tmp_path, name, batches, **kw):
    from jamun_amd.callbacks import RamachandranMetricsCallback

    cb, smp = meter_run(RamachandranMetricsCallback, tmp_path / name, rc.molecules()["AG"], batches, torch.device("cpu"), **kw)
    return cb, smp, tmp_path / name / "m" / "ramachandran"


def test_meter_on_cpu_tensors_through_the_callback(tmp_path):
    """3 chains x 130 frames, two batches: the joined trajectory's cuts 100, 200, 400 fall inside chains 0, 1 and 3 (off their ends), so the
    joined curve crosses chain boundaries."""
    from jamun_amd.callbacks import RamachandranMetricsCallback, TrajectoryMetricCallback
    from jamun_amd.features import internal_coords_host

    mol = rc.molecules()["AG"]
    chains, T, bins = 3, 130, 20
    batches = tumbling_batches(mol, torch.device("cpu"), chains, T, 2, seed=9, sigma=0.01)
    frames = [rc.chain_frames(s) for b in batches for s in b]
    rng = np.random.RandomState(4)
    reference = frames[0][rng.permutation(T)] + 0.0
    reference = np.concatenate([reference, frames[3][:50]])
    cb, smp, d = _meter_run(tmp_path, "run", batches, bins=bins, reference=reference)
    assert isinstance(cb, TrajectoryMetricCallback) and isinstance(cb, RamachandranMetricsCallback)
    assert sorted(os.listdir(d)) == sorted([f"{i}.npz" for i in range(2 * chains)] + ["joined.npz", "pairs.json", "true_traj.npz"])
    meta = json.load(open(d / "pairs.json"))
    index, pairs, labels = R.phi_psi_pairs(mol)
    assert meta["atom_indices"] == index.tolist() and meta["pairs"] == pairs.tolist() and meta["pair_labels"] == labels
    assert meta["bins"] == bins and meta["pairing"] == "reference" and meta["js_divergence"] is True

    def hist(fr, cuts):
        return R.histogram_host(internal_coords_host(fr, index).astype(np.float32), pairs, bins, cuts)

    ref_counts = hist(reference, [len(reference)])[0][0]
    assert np.array_equal(np.load(d / "true_traj.npz")["counts"], ref_counts)
    for i, fr in enumerate(frames):
        z = np.load(d / f"{i}.npz")
        seg, skipped = hist(fr, R.sample_counts(T))
        assert z["counts"].dtype == np.uint32 and z["counts"].shape == (1, bins, bins) and np.array_equal(z["counts"], seg.sum(axis=0))
        assert z["num_samples"].tolist() == [100, 130] and np.array_equal(z["skipped"], skipped.sum(axis=0))
        want = R.js_divergence_host(seg, ref_counts)
        assert z["js_divergence"].shape == (2,) and z["js_divergence_per_pair"].shape == (2, 1)
        assert np.array_equal(z["js_divergence"], want["pooled"]) and np.array_equal(z["js_divergence_per_pair"], want["per_pair"])
    joined = np.concatenate(frames)
    z = np.load(d / "joined.npz")
    cuts = R.sample_counts(len(joined))
    assert cuts == [100, 200, 400, 780] and z["num_samples"].tolist() == cuts
    seg, _ = hist(joined, cuts)
    assert np.array_equal(z["counts"], seg.sum(axis=0)) and int(z["counts"].sum()) == len(joined)
    want = R.js_divergence_host(seg, ref_counts)
    assert np.array_equal(z["js_divergence"], want["pooled"]) and np.array_equal(z["js_divergence_per_pair"], want["per_pair"])
    assert smp.fabric.logged == [{"m/js_divergence/pred_traj_joined": v} for v in
                                 (R.js_divergence_host(hist(joined[: chains * T], [100, 200, chains * T])[0], ref_counts)["pooled"][-1], want["pooled"][-1])]
    assert 0.0 < want["pooled"][-1] < np.log(2.0)
    # the same run again gives the same bytes
    _, _, d2 = _meter_run(tmp_path, "again", batches, bins=bins, reference=reference)
    assert tree(str(d)) == tree(str(d2))


def test_meter_takes_the_datasets_own_frames_as_reference(tmp_path):
    mol = rc.molecules()["AG"]
    batches = tumbling_batches(mol, torch.device("cpu"), 2, 60, 1, seed=2, sigma=0.01)
    from jamun_amd.callbacks import RamachandranMetricsCallback

    ds = CaseDataset(mol, "m")
    ds.xyz = batches[0][0]["xhat_traj"].permute(1, 0, 2).contiguous()  # [T, n, 3], as MDtrajDataset keeps its frames
    path = tmp_path / "ref.npy"
    np.save(path, ds.xyz.numpy())
    a = run(RamachandranMetricsCallback([ds], output_dir=str(tmp_path / "xyz"), bins=10), batches, StubSampler(torch.device("cpu")))
    b = run(RamachandranMetricsCallback([CaseDataset(mol, "m")], output_dir=str(tmp_path / "npy"), bins=10, reference=str(path)), batches,
               StubSampler(torch.device("cpu")))
    assert tree(str(tmp_path / "xyz")) == tree(str(tmp_path / "npy"))
    z = np.load(tmp_path / "xyz" / "m" / "ramachandran" / "0.npz")
    assert z["js_divergence"].tolist() == [0.0] and z["num_samples"].tolist() == [60]  # chain 0 IS the reference
    assert a.meters["m"].ref_counts.sum() == 60 and b.meters["m"].ref_counts.sum() == 60


def test_meter_without_reference_frames_writes_histograms_and_omits_jsd(tmp_path):
    batches = tumbling_batches(rc.molecules()["AG"], torch.device("cpu"), 2, 60, 1, seed=2, sigma=0.01)
    cb, smp, d = _meter_run(tmp_path, "noref", batches, bins=10)
    assert sorted(os.listdir(d)) == ["0.npz", "1.npz", "joined.npz", "pairs.json"]
    meta = json.load(open(d / "pairs.json"))
    assert meta["js_divergence"] is False and "omitted" in meta["note"]
    for name in ("0", "1", "joined"):
        z = np.load(d / f"{name}.npz")
        assert sorted(z.files) == ["counts", "num_samples", "skipped"] and z["counts"].sum() == (120 if name == "joined" else 60)
    assert smp.fabric.logged == [{}]


def test_residue_pairing_of_a_dipeptide_meters_nothing_and_says_so(tmp_path):
    batches = tumbling_batches(rc.molecules()["AG"], torch.device("cpu"), 1, 20, 1, seed=2, sigma=0.01)
    cb, smp, d = _meter_run(tmp_path, "residue", batches, bins=10, pairing="residue")
    assert os.listdir(d) == ["pairs.json"] and json.load(open(d / "pairs.json"))["pairs"] == []


def test_config_names_the_callback_and_the_default_run_does_not():
    from jamun_amd import config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_dir = os.path.join(root, "jamun_amd", "hydra_config", "callbacks", "sampler")
    text = open(os.path.join(cfg_dir, "ramachandran.yaml")).read()
    assert "jamun.callbacks.sampler.RamachandranPlotMetricsCallback" in text
    assert "ramachandran" not in open(os.path.join(cfg_dir, "default.yaml")).read()
    table = next(v for v in vars(config).values() if isinstance(v, dict) and "jamun.callbacks.sampler.SaveTrajectoryCallback" in v)
    assert table["jamun.callbacks.sampler.RamachandranPlotMetricsCallback"] == "jamun_amd.callbacks.RamachandranMetricsCallback"
    from jamun_amd import cmdline

    base = ["--config-dir=" + os.path.join(root, "configs"), "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=c"]
    assert "ramachandran_plot" not in cmdline.compose(base)["callbacks"]
    cfg = cmdline.compose(base + ["callbacks=[sampler/default,sampler/ramachandran]"])["callbacks"]
    assert list(cfg) == ["save_trajectory", "measure_sampling_time", "ramachandran_plot"]
    assert cfg["ramachandran_plot"]["_target_"] == "jamun.callbacks.sampler.RamachandranPlotMetricsCallback" and cfg["ramachandran_plot"]["bins"] == 100
