"""CPU tests of jamun_amd/tica.py: the host specification of the three reductions, the fit, the JS distance, the meter on the host path,
the mirrored constants and the configuration.  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

import _tica_cases as tc
from _frames_common import CaseDataset, meter_run, tree
from _traj_molecules import dipeptide
from jamun_amd import tica

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lagged_moments_host_is_the_sum_over_pairs_written_out():
    x = tc.feature_rows(23, 3)
    for lag in (1, 4, 22):
        s, m = tica.lagged_moments_host(x, lag)
        want_s, want_m = np.zeros((2, 3)), np.zeros((3, 3, 3))
        for t in range(23 - lag):
            a, b = x[t].astype(np.float64), x[t + lag].astype(np.float64)
            want_s += np.stack([a, b])
            want_m += np.stack([np.outer(a, a), np.outer(b, b), np.outer(a, b)])
        bs, bm = tc.moments_bounds(x, lag)
        assert (np.abs(s - want_s) <= 2 * bs).all() and (np.abs(m - want_m) <= 2 * bm).all()
    for bad in (0, 23, -1, 1.0, True):
        with pytest.raises(ValueError, match="lag"):
            tica.lagged_moments_host(x, bad)


def test_autocov_sums_host_over_counts_equals_a_double_loop():
    rng = np.random.RandomState(0)
    for T, max_lag in ((1, 0), (1, 3), (2, 1), (37, 36), (37, 40), (200, 25)):
        y = rng.randn(T) * 3 + 0.5
        got = tica.autocov_from_sums(tica.autocov_sums_host(y, max_lag), tica.autocov_counts(T, max_lag))
        want = tc.autocov_loop(y, max_lag)
        assert got.shape == (max_lag + 1,) and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == max(0, max_lag + 1 - T)
        k = ~np.isnan(want)
        assert np.allclose(got[k], want[k], rtol=1e-13, atol=1e-13)
        assert (tica.autocov_sums_host(y, max_lag)[T:] == 0).all()


def test_js_distance_host_equals_scipys_jensenshannon():
    from scipy.spatial.distance import jensenshannon

    rng = np.random.RandomState(1)
    for n in (1, 2, 100, 2500):
        for density in (1.0, 0.3):
            p = rng.randint(0, 50, size=n) * (rng.rand(n) < density)
            q = rng.randint(0, 50, size=n) * (rng.rand(n) < density)
            p[0] += 1
            q[-1] += 1
            assert abs(tica.js_distance_host(p, q) - jensenshannon(p, q)) <= 1e-14, (n, density)
    assert tica.js_distance_host([3, 0, 1], [3, 0, 1]) == 0.0
    assert abs(tica.js_distance_host([1, 0], [0, 1]) - np.sqrt(np.log(2.0))) <= 1e-15  # disjoint supports: the largest distance
    assert np.isnan(tica.js_distance_host([0, 0], [1, 1])) and np.isnan(tica.js_distance_host([1, 1], [0, 0]))
    with pytest.raises(ValueError, match="shape"):
        tica.js_distance_host([1, 2], [1, 2, 3])


def _reversible_statistics(x, fit, lag):
    """Of the projection z of the rows x: (C_0 of z, C_tau of z) by the reversible estimator about the model's mean."""
    z = tica.project_host(x, fit["mean"], fit["eigenvectors"])
    a, b = z[: z.shape[0] - lag], z[lag:]
    two_n = 2.0 * a.shape[0]
    return (a.T @ a + b.T @ b) / two_n, (a.T @ b + b.T @ a) / two_n


@pytest.mark.parametrize("kinetic_map", [False, True])
def test_fit_tica_on_ar1_torsions(kinetic_map):
    """Eigenvalues descending within (-1, 1] and with the fixture's gaps; the projected reference's components are mutually uncorrelated and
    the lag-tau autocorrelation of each equals its eigenvalue (an identity of the reversible estimate); the slowest component is the slowest
    torsion's; the sign convention holds."""
    x, lag = tc.fit_fixture(), tc.FIT_LAG
    s, m = tica.lagged_moments_host(x, lag)
    fit = tica.fit_tica(s, m, x.shape[0] - lag, var_cutoff=1.0, kinetic_map=kinetic_map)
    lam = fit["eigenvalues"]
    tc.check_gaps(lam)
    assert lam.shape == (6,) and (np.diff(lam) <= 0).all() and (lam > -1).all() and (lam <= 1).all()
    assert fit["d"] == 6 and fit["eigenvectors"].shape == (6, 6) and fit["cumulative_variance"][-1] == pytest.approx(1.0, abs=1e-14)
    c0, ct = _reversible_statistics(x, fit, lag)
    scale = lam if kinetic_map else np.ones(6)
    assert np.allclose(c0, np.diag(scale * scale), atol=1e-10)      # uncorrelated, variance 1 (lambda^2 on the kinetic map)
    assert np.allclose(ct, np.diag(lam * scale * scale), atol=1e-10)  # autocorrelation at the lag = the eigenvalue
    assert abs(lam[0] - tc.FIT_RHOS[0] ** lag) < 0.05               # the slowest torsion's linear mode, rho^tau
    u = fit["eigenvectors"]
    assert (np.abs(u[:2, 0]) ** 2).sum() > 0.9 * (u[:, 0] ** 2).sum()  # ... which lives on that torsion's (cos, sin) pair
    assert (u[np.argmax(np.abs(u), axis=0), np.arange(6)] > 0).all()
    # the default cutoff keeps the smallest d that reaches 95 % of sum lambda^2
    cut = tica.fit_tica(s, m, x.shape[0] - lag, kinetic_map=kinetic_map)
    cv = cut["cumulative_variance"]
    assert 1 <= cut["d"] < 6 and cv[cut["d"] - 1] >= 0.95 and (cut["d"] == 1 or cv[cut["d"] - 2] < 0.95)
    assert np.array_equal(cut["eigenvectors"], u[:, : cut["d"]])


def test_fit_tica_drops_directions_without_variance_and_refuses_bad_moments():
    x = np.array(tc.fit_fixture())
    x = np.concatenate([x, x[:, :1] * 2.0, np.full((x.shape[0], 1), 0.25, dtype=np.float32)], axis=1)  # a dependent and a constant column
    s, m = tica.lagged_moments_host(x, tc.FIT_LAG)
    fit = tica.fit_tica(s, m, x.shape[0] - tc.FIT_LAG, var_cutoff=1.0)
    ref = tica.fit_tica(*tica.lagged_moments_host(tc.fit_fixture(), tc.FIT_LAG), tc.FIT_T - tc.FIT_LAG, var_cutoff=1.0)
    assert fit["eigenvalues"].shape == (6,) and np.allclose(fit["eigenvalues"], ref["eigenvalues"], atol=1e-9)
    with pytest.raises(ValueError, match="not finite"):
        tica.fit_tica(s * np.nan, m, 10)
    with pytest.raises(ValueError, match="epsilon"):
        tica.fit_tica(np.zeros((2, 2)), np.zeros((3, 2, 2)), 10)
    with pytest.raises(ValueError, match="expected sums"):
        tica.fit_tica(np.zeros((2, 2)), np.zeros((3, 2, 3)), 10)


def test_moments_of_two_trajectories_summed_fit_the_list_not_the_concatenation():
    lag = tc.FIT_LAG
    a, b = tc.fit_fixture(seed=3, T=2500), tc.fit_fixture(seed=4, T=2000)
    (sa, ma), (sb, mb) = tica.lagged_moments_host(a, lag), tica.lagged_moments_host(b, lag)
    n = a.shape[0] + b.shape[0] - 2 * lag
    fit = tica.fit_tica(sa + sb, ma + mb, n, var_cutoff=1.0)
    # the list, written out: every pair of a and every pair of b, none across the seam
    pairs = [(t[i], t[i + lag]) for t in (a.astype(np.float64), b.astype(np.float64)) for i in range(t.shape[0] - lag)]
    x0, xt = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    want = tica.fit_tica(np.stack([x0.sum(0), xt.sum(0)]), np.stack([x0.T @ x0, xt.T @ xt, x0.T @ xt]), len(pairs), var_cutoff=1.0)
    assert len(pairs) == n and np.allclose(fit["eigenvalues"], want["eigenvalues"], atol=1e-11) and np.allclose(fit["eigenvectors"], want["eigenvectors"], atol=1e-8)
    cat = np.concatenate([a, b])
    other = tica.fit_tica(*tica.lagged_moments_host(cat, lag), cat.shape[0] - lag, var_cutoff=1.0)
    assert np.abs(other["eigenvalues"] - fit["eigenvalues"]).max() > 1e-6  # (the concatenation has `lag` pairs across the seam)


def test_feature_table_is_pyemmas_backbone_and_sidechain_torsions():
    index, labels = tica.tica_feature_table(dipeptide(), "all")
    assert labels == ["COS(PHI 0 GLY 1)", "SIN(PHI 0 GLY 1)", "COS(PSI 0 ALA 0)", "SIN(PSI 0 ALA 0)"]  # (no omega; this dipeptide has no chi)
    assert index.tolist() == [[3, 5, 6, 7], [0, 1, 3, 5]] and index.dtype == np.int32
    assert tica.tica_feature_table(dipeptide(), "backbone")[1] == labels
    with pytest.raises(ValueError, match="features"):
        tica.tica_feature_table(dipeptide(), "distances")


def test_native_constants_mirror_the_header():
    from jamun_amd import native

    hdr = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_internal.h")).read()
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))
    assert (native.TICA_MAX_WIDTH, native.TICA_MAX_ACF_LAG, native.TICA_SLICE, native.TICA_TILE) == (
        macro("JAMUN_TICA_MAX_WIDTH"), macro("JAMUN_TICA_MAX_ACF_LAG"), macro("JAMUN_TICA_SLICE"), macro("JAMUN_TICA_TILE")) == (128, 4096, 1024, 32)


def test_wrappers_refuse_bad_arguments_before_anything_needs_a_gpu():
    from jamun_amd import native

    x = torch.zeros(10, 4)
    with pytest.raises(ValueError, match="lag"):
        native.lagged_moments(x, 10)
    with pytest.raises(ValueError, match="lag"):
        native.lagged_moments(x, 0)
    with pytest.raises(ValueError, match="feature columns"):
        native.lagged_moments(torch.zeros(10, 129), 1)
    with pytest.raises(ValueError, match="feature columns"):
        native.project_frames(torch.zeros(10, 0), np.zeros(0), np.zeros((0, 0)))
    with pytest.raises(ValueError, match="mean must have shape"):
        native.project_frames(x, np.zeros(4), np.zeros((4, 5)))
    with pytest.raises(ValueError, match="mean must have shape"):
        native.project_frames(x, np.zeros(3), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="max_lag"):
        native.autocov_sums(torch.zeros(10, dtype=torch.float64), 4097)
    with pytest.raises(ValueError, match="max_lag"):
        native.autocov_sums(torch.zeros(10, dtype=torch.float64), -1)
    with pytest.raises(RuntimeError, match="on the GPU"):
        native.lagged_moments(x, 1)


def test_config_names_the_callback_and_the_default_run_does_not():
    from jamun_amd import callbacks, cmdline, config

    cfg_dir = os.path.join(ROOT, "jamun_amd", "hydra_config", "callbacks", "sampler")
    assert "tica" not in open(os.path.join(cfg_dir, "default.yaml")).read()
    table = next(v for v in vars(config).values() if isinstance(v, dict) and "jamun.callbacks.sampler.SaveTrajectoryCallback" in v)
    assert table["jamun.callbacks.sampler.TICAMetricsCallback"] == "jamun_amd.callbacks.TICAMetricsCallback"
    base = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=c"]
    assert "tica" not in cmdline.compose(base)["callbacks"]
    cfg = cmdline.compose(base + ["callbacks=[sampler/default,sampler/tica]"])["callbacks"]
    assert list(cfg) == ["save_trajectory", "measure_sampling_time", "tica"]
    entry = cfg["tica"]
    assert entry["_target_"] == "jamun.callbacks.sampler.TICAMetricsCallback"
    assert (entry["lag"], entry["max_acf_lag"], entry["features"], entry["bins_1d"], entry["bins_2d"], entry["kinetic_map"]) == (1000, 1000, "all", 100, 50, True)
    cb = config.instantiate({k: v for k, v in entry.items() if k != "datasets"}, datasets=[CaseDataset(dipeptide(), "m")])
    assert isinstance(cb, callbacks.TICAMetricsCallback)
    meter = cb.meters["m"]
    assert (meter.lag, meter.max_acf_lag, meter.var_cutoff, meter.epsilon, meter.width) == (1000, 1000, 0.95, 1e-6, 4)


# ---- the meter on the host path ------------------------------------------------------------------------------------------------------------------

def _run(root, batches, xyz=None, **kw):
    from jamun_amd.callbacks import TICAMetricsCallback

    kw = dict(dict(lag=tc.METER_LAG, max_acf_lag=tc.METER_ACF_LAG), **kw)
    cb, smp = meter_run(TICAMetricsCallback, root, dipeptide(), batches, torch.device("cpu"), xyz=xyz, **kw)
    return cb, smp, root / "m" / "tica"


def test_meter_on_the_host_path_writes_the_file_set(tmp_path):
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    cb, smp, d = _run(tmp_path, batches, xyz=ref)
    assert sorted(os.listdir(d)) == sorted([f"{i}.npz" for i in range(6)] + ["joined.npz", "model.json", "model.npz", "true_traj.npz"])
    info = json.load(open(d / "model.json"))
    assert info["note"] is None and info["lag"] == tc.METER_LAG and info["d"] == 3 and len(info["feature_labels"]) == 4 and info["estimator"] == "reversible"
    model = np.load(d / "model.npz")
    tc.check_gaps(model["eigenvalues"])
    assert model["mean"].shape == (4,) and model["eigenvectors"].shape == (4, 3) and model["cumulative_variance"].shape == (4,)
    true = np.load(d / "true_traj.npz")
    R, T, K = tc.METER_REFERENCE_T, tc.METER_CHAIN_T, tc.METER_ACF_LAG
    assert true["tic01"].shape == (R, 2) and true["autocov"].shape == (K + 1,) and int(true["num_frames"].item()) == R
    # the files are what the specification gives for the chain's own frames
    meter = cb.meters["m"]
    frames = batches[1][2]["xhat_traj"].permute(1, 0, 2).numpy()
    x = meter._features(frames)
    proj = tica.project_host(x, model["mean"], model["eigenvectors"])
    z = np.load(d / "5.npz")
    assert sorted(z.files) == ["autocov", "js_distance_tic0", "js_distance_tic01", "nonfinite_frames", "num_frames", "tic01"]
    assert np.array_equal(z["tic01"], proj[:, :2]) and int(z["num_frames"].item()) == T and int(z["nonfinite_frames"].item()) == 0
    assert np.allclose(z["autocov"], tc.autocov_loop(proj[:, 0], K), rtol=1e-12, atol=1e-14)
    want = tica.tica_js_distances(proj[:, :2], true["tic01"], 100, 50)
    assert float(z["js_distance_tic0"].item()) == want["js_distance_tic0"] and float(z["js_distance_tic01"].item()) == want["js_distance_tic01"]
    assert 0.0 < want["js_distance_tic0"] < np.sqrt(np.log(2.0))
    # the joined trajectory: frames concatenated, the autocovariance from summed sums over summed counts
    j = np.load(d / "joined.npz")
    chains = [np.load(d / f"{i}.npz") for i in range(6)]
    assert np.array_equal(j["tic01"], np.concatenate([c["tic01"] for c in chains])) and int(j["num_frames"].item()) == 6 * T
    counts = tica.autocov_counts(T, K)
    assert np.allclose(j["autocov"], sum(c["autocov"] * counts for c in chains) / (6 * counts), rtol=1e-12, atol=1e-14)
    whole = tc.autocov_loop(j["tic01"][:, 0], K)
    assert np.abs(whole[1:] - j["autocov"][1:]).max() > 1e-9  # (not the autocovariance of the concatenation)
    assert smp.fabric.logged[-1] == {"m/tica/js_distance_tic0_joined": float(j["js_distance_tic0"].item())} and len(smp.fabric.logged) == 2
    # the same run again gives the same bytes
    _run(tmp_path / "again", batches, xyz=ref)
    assert tree(str(d)) == tree(str(tmp_path / "again" / "m" / "tica"))


def test_meter_counts_non_finite_frames_and_leaves_them_out(tmp_path):
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    clean = batches[0][:2]
    dirty = [dict(s, xhat_traj=s["xhat_traj"].clone()) for s in clean]
    dirty[1]["xhat_traj"][7, 11, 2] = float("nan")  # atom 7 (C of GLY) in frame 11: phi of that frame
    dirty[1]["xhat_traj"][0, 200, 0] = float("inf")  # atom 0 (N of ALA) in frame 200: psi
    _, _, d0 = _run(tmp_path / "clean", [clean], xyz=ref)
    _, smp, d1 = _run(tmp_path / "dirty", [dirty], xyz=ref)
    a, b = np.load(d0 / "1.npz"), np.load(d1 / "1.npz")
    assert int(b["nonfinite_frames"].item()) == 2 and np.isnan(b["autocov"]).all() and not np.isnan(a["autocov"]).any()
    bad = ~np.isfinite(b["tic01"]).all(axis=1)
    assert np.flatnonzero(bad).tolist() == [11, 200] and np.array_equal(a["tic01"][~bad], b["tic01"][~bad])
    assert np.isfinite(float(b["js_distance_tic0"].item())) and float(b["js_distance_tic0"].item()) != float(a["js_distance_tic0"].item())
    j0, j1 = np.load(d0 / "joined.npz"), np.load(d1 / "joined.npz")
    assert int(j1["nonfinite_frames"].item()) == 2 and int(j1["num_frames"].item()) == 2 * tc.METER_CHAIN_T
    assert np.array_equal(j1["autocov"], np.load(d1 / "0.npz")["autocov"]) and not np.array_equal(j0["autocov"], j1["autocov"])  # chain 1 left out
    assert np.isfinite(list(smp.fabric.logged[-1].values())[0])


@pytest.mark.parametrize("case", ["none", "short", "nan"])
def test_meter_without_a_usable_reference_writes_the_note_only(tmp_path, case):
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    xyz = {"none": None, "short": ref[: tc.METER_LAG], "nan": ref.clone()}[case]
    if case == "nan":
        xyz[900, 3, 1] = float("nan")
    cb, smp, d = _run(tmp_path, batches[:1], xyz=xyz)
    assert os.listdir(d) == ["model.json"]
    info = json.load(open(d / "model.json"))
    assert info["d"] is None and {"none": "no reference frames", "short": "no lag pair", "nan": "non-finite feature"}[case] in info["note"]
    assert smp.fabric.logged == [{}] and cb.meters["m"].compute() == {}


def test_meter_overlaps_the_reference_chunks_by_the_lag(tmp_path, monkeypatch):
    """Chunks of 400 and of 1 pair give the moments of the whole reference: no pair is lost at a boundary, none counted twice."""
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    _, _, whole = _run(tmp_path / "whole", batches[:1], xyz=ref)
    monkeypatch.setattr(tica.TICAMetrics, "REFERENCE_CHUNK", 400)
    _, _, parts = _run(tmp_path / "parts", batches[:1], xyz=ref)
    a, b = np.load(whole / "model.npz"), np.load(parts / "model.npz")
    for k in ("mean", "eigenvalues", "eigenvectors"):
        assert np.abs(a[k] - b[k]).max() <= tc.METER_TOLERANCE[k], k  # (the same pairs added in another order: inside the moments' rounding)
    assert np.abs(np.load(whole / "true_traj.npz")["tic01"] - np.load(parts / "true_traj.npz")["tic01"]).max() <= tc.METER_TOLERANCE["tic01"]


def test_meter_arguments_and_the_device_message(tmp_path):
    ds = CaseDataset(dipeptide(), "m")
    for kw in (dict(lag=0), dict(max_acf_lag=-1), dict(bins_1d=0), dict(lag=2.5), dict(features="distances"), dict(device="gpu")):
        with pytest.raises(ValueError):
            tica.TICAMetrics(ds, output_dir=str(tmp_path), **kw)
    with pytest.raises(ValueError, match="no molecule"):
        tica.TICAMetrics(CaseDataset(None, "m"))
    ref, batches = tc.meter_fixture(dipeptide(), torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"TICAMetrics\(device='device'\) needs float32 sample tensors on a GPU"):
        _run(tmp_path, batches[:1], xyz=ref, device="device")


def test_the_meter_tolerances_are_ten_times_what_the_fixture_shows():
    """`_tica_cases.METER_TOLERANCE` against a fresh measurement: the constants stay what the fixture gives (within a factor 2: the draws
    of the signs are the same, the eigen-solver's rounding may differ between machines)."""
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    meter = tica.TICAMetrics(CaseDataset(mol, "m"), lag=tc.METER_LAG, max_acf_lag=tc.METER_ACF_LAG, device="host")
    seen = tc.measure_meter_sensitivity(meter._features(ref), [meter._features(s["xhat_traj"].permute(1, 0, 2)) for b in batches for s in b])
    assert set(seen) == set(tc.METER_OBSERVED)
    for k, v in seen.items():
        assert 0.5 * tc.METER_OBSERVED[k] <= v <= 2.0 * tc.METER_OBSERVED[k], (k, v, tc.METER_OBSERVED[k])
        assert tc.METER_TOLERANCE[k] == 10.0 * tc.METER_OBSERVED[k]
