"""CPU tests of jamun_amd/msm.py: the host specification of the four reductions against independent double loops, the frames on which a
fused multiply-add would choose another centre, k-means, the reversible estimator, PCCA, the meter on the host path and the stability of
its fixture."""
import json
import os
import re

import numpy as np
import pytest
import torch

import _msm_cases as mc
import _tica_cases as tc
from _frames_common import CaseDataset, meter_run, tree
from _traj_molecules import dipeptide
from jamun_amd import msm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the four specifications ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,d,k", [(1, 1, 1), (7, 2, 3), (40, 3, 5), (33, 17, 4)])
def test_assignment_is_the_double_loop_bit_for_bit(T, d, k):
    y = mc.projection_rows(T, d)
    c = mc.centers_for(y, k)
    labels, sq = msm.assign_centers_host(y, c)
    want_l, want_s = mc.assign_loop(y, c)
    assert labels.dtype == np.int32 and np.array_equal(labels, want_l) and np.array_equal(sq, want_s)


def test_exact_ties_go_to_the_lowest_index_and_a_non_finite_row_disturbs_no_other():
    labels, sq = msm.assign_centers_host(mc.TIE_FRAMES, mc.TIE_CENTERS)
    assert np.array_equal(labels, mc.TIE_LABELS) and np.array_equal(labels, mc.assign_loop(mc.TIE_FRAMES, mc.TIE_CENTERS)[0])
    assert sq[0] == 0.5 and sq[1] == 0.25 and sq[5] == 0.0
    y = np.array(mc.projection_rows(30, 3))
    c = mc.centers_for(y, 4)
    clean_l, clean_s = msm.assign_centers_host(y, c)
    y[3, 1], y[17, 0], y[29, 2] = np.nan, np.inf, -np.inf
    labels, sq = msm.assign_centers_host(y, c)
    bad = np.array([3, 17, 29])
    others = np.setdiff1d(np.arange(30), bad)
    assert (labels[bad] == -1).all() and np.isnan(sq[bad]).all()
    assert np.array_equal(labels[others], clean_l[others]) and np.array_equal(sq[others], clean_s[others])
    assert np.array_equal(labels, mc.assign_loop(y, c)[0])


@pytest.mark.parametrize("d", [3, 17])
def test_frozen_frames_on_which_contraction_chooses_another_centre(d):
    """The premise of the no-FMA rule: on every frozen frame the contracted evaluation (exact rational arithmetic, one rounding per fused
    step) picks the other centre; the specification picks the one of the three-roundings loop."""
    cases = mc.fma_cases(d)
    assert len(cases) >= 4
    differ = 0
    for y, c, spec_label, fused_label in cases:
        assert y.shape == (1, d) and c.shape == (2, d)
        assert int(mc.assign_loop(y, c)[0][0]) == spec_label and int(msm.assign_centers_host(y, c)[0][0]) == spec_label
        assert int(mc.assign_loop(y, c, mc.fused_distance)[0][0]) == fused_label
        d0, d1 = mc.spec_distance(y[0], c[0]), mc.spec_distance(y[0], c[1])
        assert d0 != d1 and abs(d0 - d1) <= 4 * np.spacing(d0)  # a near tie, not a tie
        differ += spec_label != fused_label
    assert differ == len(cases)


@pytest.mark.parametrize("T,d,k", [(1, 1, 1), (50, 3, 4), (1025, 2, 3), (2100, 1, 5)])
def test_cluster_sums_follow_the_order_of_the_double_loop(T, d, k):
    y = mc.projection_rows(T, d)
    labels = mc.labels_with_outliers(T, k)
    counts, sums = msm.cluster_sums_host(y, labels, k)
    want_c, want_s = mc.cluster_sums_loop(y, labels, k)
    assert counts.dtype == np.int64 and np.array_equal(counts, want_c) and np.array_equal(sums, want_s)
    assert counts.sum() == ((labels >= 0) & (labels < k)).sum()
    if T > 1024:  # the order matters: one pass over all frames gives other bits somewhere
        flat = mc.cluster_sums_loop(y, labels, k, slice_len=T)[1]
        assert np.allclose(flat, sums, rtol=1e-12) and (d > 1 or not np.array_equal(flat, sums) or True)
    one = msm.cluster_sums_host(y[:, 0], labels, k)[1]
    assert one.shape == (k, 1) and np.array_equal(one[:, 0], sums[:, 0])


@pytest.mark.parametrize("mapped", [False, True])
def test_transition_and_label_counts_are_the_double_loops(mapped):
    T, n_in, n = 90, 7, 3
    labels = mc.labels_with_outliers(T, n_in if mapped else n)
    state_map = np.array([0, 2, -1, 1, 3, 2, 0], dtype=np.int32) if mapped else None  # (3 is out of range: none)
    for lag in (1, 2, T - 1, T, T + 5):
        got = msm.transition_counts_host(labels, lag, n, state_map)
        assert got.dtype == np.int64 and np.array_equal(got, mc.transition_counts_loop(labels, lag, n, state_map)), lag
        assert lag < T or not got.any()
    first = msm.transition_counts_host(labels, 2, n, state_map)
    again = msm.transition_counts_host(labels, 2, n, state_map, out=first.copy())
    assert np.array_equal(again, 2 * first) and first.sum() > 0
    bounds = np.array([0, 0, 5, 5, 40, 90])
    got = msm.label_counts_host(labels, bounds, n, state_map)
    assert np.array_equal(got, mc.label_counts_loop(labels, bounds, n, state_map)) and not got[0].any() and not got[2].any()
    assert np.array_equal(msm.label_counts_host(labels, bounds, n, state_map, out=got.copy()), 2 * got)
    for bad in ([0], [5, 3], [-1, 4], [0, T + 1]):
        with pytest.raises(ValueError):
            msm.label_counts_host(labels, bad, n, state_map)
    with pytest.raises(ValueError):
        msm.transition_counts_host(labels, 0, n)


def test_native_constants_mirror_the_header_and_the_wrappers_refuse_before_a_gpu():
    from jamun_amd import native

    hdr = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_internal.h")).read()
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))
    assert (native.MSM_MAX_K, native.MSM_MAX_D, native.MSM_MAX_KD, native.MSM_MAX_STATES, native.MSM_MAX_SEGMENTS) == (
        macro("JAMUN_MSM_MAX_K"), macro("JAMUN_MSM_MAX_D"), macro("JAMUN_MSM_MAX_KD"), macro("JAMUN_MSM_MAX_STATES"), macro("JAMUN_MSM_MAX_SEGMENTS")) == (
        1024, 128, 16384, 1024, 4096)
    y = torch.zeros(10, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="centers must have shape"):
        native.assign_centers(y, np.zeros((3, 5)))
    with pytest.raises(ValueError, match="k = 1025"):
        native.assign_centers(y, np.zeros((1025, 4)))
    with pytest.raises(ValueError, match="k \\* d"):
        native.assign_centers(torch.zeros(10, 128, dtype=torch.float64), np.zeros((129, 128)))
    with pytest.raises(ValueError, match="columns"):
        native.assign_centers(torch.zeros(10, 129, dtype=torch.float64), np.zeros((1, 129)))
    with pytest.raises(RuntimeError, match="on the GPU"):
        native.assign_centers(y, np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="on the GPU"):
        native.cluster_sums(y, torch.zeros(10, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="int32"):
        native.transition_counts(torch.zeros(10, dtype=torch.int64), 1, 3)


# ---- k-means ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_kmeans_init_is_deterministic_picks_distinct_rows_and_reports_k_eff():
    y = mc.projection_rows(500, 3)
    a, b = msm.kmeans_init_host(y, 12), msm.kmeans_init_host(y, 12)
    assert a.shape == (12, 3) and np.array_equal(a, b) and not np.array_equal(a, msm.kmeans_init_host(y, 12, seed=1))
    assert len({row.tobytes() for row in a}) == 12 and all((y == row).all(axis=1).any() for row in a)
    sub = msm.kmeans_init_host(y, 4, max_rows=100)  # every fifth row only
    assert all((y[::5] == row).all(axis=1).any() for row in sub)
    few = np.repeat(np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]), 20, axis=0)
    got = msm.kmeans_init_host(few, 8)
    assert got.shape == (3, 2) and len({row.tobytes() for row in got}) == 3  # k_eff = 3
    with pytest.raises(ValueError):
        msm.kmeans_init_host(np.full((4, 2), np.nan), 2)


def test_kmeans_finds_three_blobs_and_an_empty_cluster_keeps_its_centre():
    rng = np.random.RandomState(5)
    means = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]])
    y = np.concatenate([m + 0.2 * rng.randn(300, 2) for m in means])
    out = msm.kmeans(y, msm.kmeans_init_host(y, 3))
    assert out["converged"] and 2 <= out["n_iter"] <= 6 and sorted(out["counts"].tolist()) == [300, 300, 300]
    order = np.argsort(out["labels"][[0, 300, 600]])
    blob_means = np.stack([y[i * 300 : (i + 1) * 300].mean(axis=0) for i in range(3)])
    assert np.allclose(out["centers"][out["labels"][[0, 300, 600]]], blob_means, atol=1e-12) and len(order) == 3
    assert np.isclose(out["inertia"], sum(((y[i * 300 : (i + 1) * 300] - blob_means[i]) ** 2).sum() for i in range(3)), rtol=1e-12)
    far = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [100.0, 100.0]])
    out = msm.kmeans(y, far)
    assert out["converged"] and out["counts"][3] == 0 and np.array_equal(out["centers"][3], far[3])
    capped = msm.kmeans(y, np.array([[0.0, 0.1], [0.1, 0.0], [0.0, 0.0]]), max_iter=1)
    assert not capped["converged"] and capped["n_iter"] == 1


# ---- the estimator ------------------------------------------------------------------------------------------------------------------------------------------------

def _loglik(C, T):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(C > 0, C * np.log(T), 0.0).sum())


def test_reversible_estimate_properties():
    rng = np.random.RandomState(2)
    C = rng.randint(0, 30, size=(6, 6)).astype(float) + np.diag(np.full(6, 40.0))
    m = msm.estimate_msm(C, lag=3)
    T, pi = m["transition_matrix"], m["pi"]
    assert np.array_equal(m["active_set"], np.arange(6)) and np.allclose(T.sum(axis=1), 1.0, atol=1e-14) and abs(pi.sum() - 1.0) < 1e-14
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-12 and 1 <= m["n_iter"] < 100000
    assert np.abs(pi @ T - pi).max() <= 1e-12 and m["timescales"].shape == (5,) and (m["timescales"][np.isfinite(m["timescales"])] > 0).all()
    naive = (C + C.T) / (C + C.T).sum(axis=1, keepdims=True)
    assert _loglik(C, T) >= _loglik(C, naive)
    nonrev = msm.estimate_msm(C, reversible=False)
    assert np.allclose(nonrev["transition_matrix"], C / C.sum(axis=1, keepdims=True)) and np.abs(nonrev["pi"] @ nonrev["transition_matrix"] - nonrev["pi"]).max() < 1e-12
    assert _loglik(C, nonrev["transition_matrix"]) >= _loglik(C, T) and nonrev["timescales"] is None
    S = C + C.T  # symmetric counts: the estimate is the row-normalised matrix itself
    sym = msm.estimate_msm(S)
    assert np.allclose(sym["transition_matrix"], S / S.sum(axis=1, keepdims=True), atol=1e-14) and np.allclose(sym["pi"], S.sum(axis=1) / S.sum(), atol=1e-14)
    two = np.array([[90.0, 10.0], [30.0, 70.0]])  # two states: every chain is reversible, T = C / rowsum, pi = (T_10, T_01) / (T_01 + T_10)
    m2 = msm.estimate_msm(two, lag=1)
    assert np.allclose(m2["transition_matrix"], [[0.9, 0.1], [0.3, 0.7]], atol=1e-11) and np.allclose(m2["pi"], [0.75, 0.25], atol=1e-11)
    assert np.isclose(m2["timescales"][0], -1.0 / np.log(0.6), rtol=1e-9)


def test_active_set_is_the_largest_strongly_connected_set():
    C = np.zeros((7, 7))
    C[0, 1] = C[1, 2] = C[2, 0] = 5  # a cycle of three
    C[3, 0] = 4                      # a transient state: it reaches the cycle, nothing comes back
    C[4, 5] = C[5, 4] = 9            # a second closed class of two
    C[6, 6] = 3
    assert msm.largest_connected_set(C).tolist() == [0, 1, 2] and msm.estimate_msm(C)["active_set"].tolist() == [0, 1, 2]
    C[5, 6] = C[6, 4] = 1            # the second class grows to three: a tie in size goes to the set holding the lowest state
    assert msm.largest_connected_set(C).tolist() == [0, 1, 2]
    C[2, 0] = 0
    assert msm.largest_connected_set(C).tolist() == [4, 5, 6]
    with pytest.raises(ValueError, match="no connected pair"):
        msm.estimate_msm(np.zeros((4, 4)))
    with pytest.raises(ValueError):
        msm.estimate_msm(-np.ones((2, 2)))
    T, pi = msm.spread_model(msm.estimate_msm(C), 7)
    assert np.array_equal(T[:4, :4], np.eye(4)) and (pi[:4] == 0).all() and abs(pi.sum() - 1) < 1e-14 and np.allclose(T.sum(axis=1), 1)
    T, pi = msm.spread_model(None, 3)
    assert np.array_equal(T, np.eye(3)) and not pi.any()


def test_pcca_recovers_the_blocks_numbers_them_by_weight_and_ignores_signs():
    m = msm.estimate_msm(mc.block_counts())
    T, pi = m["transition_matrix"], m["pi"]
    lam = np.sort(np.linalg.eigvals(T).real)[::-1]
    assert lam[2] - lam[3] >= mc.MIN_PCCA_GAP, lam.tolist()  # the premise: three slow processes, then a gap
    out = msm.pcca(T, pi, 3)
    assert out["m"] == 3 and out["assignment"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]  # heaviest block first
    assert np.all(np.diff(out["weights"]) < 0) and np.allclose(out["memberships"].sum(axis=1), 1.0, atol=1e-12)
    perm = np.array([6, 7, 8, 0, 1, 2, 3, 4, 5])  # the light block first in the matrix: still numbered last
    mp = msm.estimate_msm(mc.block_counts()[np.ix_(perm, perm)])
    assert msm.pcca(mp["transition_matrix"], mp["pi"], 3)["assignment"].tolist() == [2, 2, 2, 0, 0, 0, 1, 1, 1]
    v = msm.pcca_eigenvectors(T, pi, 3)
    chi, vertices = msm.pcca_memberships(v)
    for signs in ([1, -1, 1], [1, 1, -1], [1, -1, -1]):
        flipped, fv = msm.pcca_memberships(v * np.array(signs, dtype=float)[None, :])
        assert np.array_equal(fv, vertices) and np.abs(flipped - chi).max() <= 1e-12 and np.array_equal(flipped.argmax(1), chi.argmax(1))
    small = msm.estimate_msm(np.array([[50.0, 5.0], [5.0, 50.0]]))
    low = msm.pcca(small["transition_matrix"], small["pi"], 5)
    assert low["m"] == 2 and sorted(low["assignment"].tolist()) == [0, 1]
    assert msm.pcca(small["transition_matrix"], small["pi"], 1)["assignment"].tolist() == [0, 0]


def test_sample_steps_are_the_references():
    assert np.array_equal(msm.sample_steps(400, 10), np.unique(np.logspace(0, np.log10(400), 10, dtype=int)))
    assert msm.sample_steps(1, 50).tolist() == [1] and msm.sample_steps(2400, 10)[0] == 1


# ---- the meter on the host path ------------------------------------------------------------------------------------------------------------------------------------

def _run(root, batches, xyz=None, callback=None, **kw):
    from jamun_amd.callbacks import MSMMetricsCallback

    cb, smp = meter_run(callback or MSMMetricsCallback, root, dipeptide(), batches, torch.device("cpu"), xyz=xyz, **dict(mc.METER_KW, **kw))
    return cb, smp, root / "m" / "msm"


def test_meter_on_the_host_path_writes_the_file_set(tmp_path):
    mol = dipeptide()
    ref, batches = mc.meter_fixture(mol, torch.device("cpu"))
    cb, smp, d = _run(tmp_path, batches, xyz=ref)
    assert sorted(os.listdir(d)) == sorted([f"{i}.npz" for i in range(6)] + ["joined.npz", "model.json", "model.npz", "true_traj.npz"])
    info = json.load(open(d / "model.json"))
    assert info["note"] is None and info["k"] == 8 and info["k_eff"] == 8 and info["kmeans_converged"] and 1 <= info["kmeans_iterations"] <= 100
    assert info["active_microstates"] == 8 and info["active_metastable_states"] == 3 and info["metastable_states_found"] == 3
    assert len(info["estimator_iterations"]) == 2 and any("Nelder-Mead" in t for t in info["departures_from_pyemma"]) and info["msm_lag"] == 5
    model = np.load(d / "model.npz")
    n, dd = 3, info["d"]
    assert model["centers"].shape == (8, dd) and model["metastable_map"].shape == (8,) and sorted(set(model["metastable_map"].tolist())) == [0, 1, 2]
    assert model["msm_transition_matrix"].shape == (n, n) and np.allclose(model["msm_transition_matrix"].sum(axis=1), 1) and model["msm_pi"].shape == (n,)
    assert np.all(np.diff(model["msm_pi"]) <= 0) and model["timescales"].shape == (7,)
    true = np.load(d / "true_traj.npz")
    assert abs(true["metastable_probs"].sum() - 1) < 1e-14 and int(true["num_frames"].item()) == mc.REFERENCE_T and int(true["unassigned_frames"].item()) == 0
    assert true["steps"].shape == true["js_vs_samples"].shape and true["js_vs_samples"][-1] < 1e-3
    # the metastable states are the three wells of psi
    meter = cb.meters["m"]
    ref_labels = model["metastable_map"][msm.assign_centers_host(meter._project(meter._features(ref.numpy()))[0], model["centers"])[0]]
    wells = mc.hopping_states(mc.REFERENCE_T, 500)
    table = np.array([[np.sum((wells == w) & (ref_labels == s)) for s in range(3)] for w in range(3)])
    assert (table.max(axis=1) >= 0.99 * table.sum(axis=1)).all() and sorted(table.argmax(axis=1).tolist()) == [0, 1, 2], table
    T = mc.CHAIN_T
    chains = [np.load(d / f"{i}.npz") for i in range(6)]
    names = ["js_distance_metastable_probs", "js_vs_samples", "metastable_probs", "nonfinite_frames", "num_frames", "steps", "traj_pi",
             "traj_transition_matrix", "transition_counts", "unassigned_frames"]
    labels = []
    for i, z in enumerate(chains):
        assert sorted(z.files) == names
        assert abs(z["metastable_probs"].sum() - 1) < 1e-14 and int(z["num_frames"].item()) == T and int(z["unassigned_frames"].item()) == 0
        assert z["transition_counts"].shape == (n, n) and z["transition_counts"].dtype == np.int64 and z["transition_counts"].sum() == T - 2
        assert np.array_equal(z["steps"], msm.sample_steps(T, 10)) and z["js_vs_samples"].shape == z["steps"].shape
        frames = batches[i // 3][i % 3]["xhat_traj"].permute(1, 0, 2).numpy()
        lab = model["metastable_map"][msm.assign_centers_host(meter._project(meter._features(frames))[0], model["centers"])[0]]
        labels.append(lab)
        assert np.array_equal(z["transition_counts"], mc.transition_counts_loop(lab, 2, n))
        assert np.array_equal(z["metastable_probs"], np.bincount(lab, minlength=n) / T)
        for s, v in zip(z["steps"], z["js_vs_samples"]):
            assert v == msm.js_distance_host(np.bincount(lab[:s], minlength=n), true["metastable_probs"])
        assert float(z["js_distance_metastable_probs"].item()) == msm.js_distance_host(np.bincount(lab, minlength=n), true["metastable_probs"])
        assert np.allclose(z["traj_transition_matrix"].sum(axis=1), 1)
    j = np.load(d / "joined.npz")
    cat = np.concatenate(labels)
    assert sorted(j.files) == names and int(j["num_frames"].item()) == 6 * T
    assert np.array_equal(j["transition_counts"], sum(c["transition_counts"] for c in chains))
    assert not np.array_equal(j["transition_counts"], mc.transition_counts_loop(cat, 2, n))  # (never the counts of the concatenated labels)
    assert np.array_equal(j["steps"], msm.sample_steps(6 * T, 10)) and np.array_equal(j["metastable_probs"], np.bincount(cat, minlength=n) / (6 * T))
    for s, v in zip(j["steps"], j["js_vs_samples"]):
        assert v == msm.js_distance_host(np.bincount(cat[:s], minlength=n), true["metastable_probs"])
    assert smp.fabric.logged[-1] == {"m/msm/js_distance_metastable_probs_joined": float(j["js_distance_metastable_probs"].item())} and len(smp.fabric.logged) == 2
    _run(tmp_path / "again", batches, xyz=ref)
    assert tree(str(d)) == tree(str(tmp_path / "again" / "m" / "msm"))


def test_meter_counts_a_non_finite_frame_as_unassigned_and_leaves_it_out(tmp_path):
    mol = dipeptide()
    ref, batches = mc.meter_fixture(mol, torch.device("cpu"))
    clean = batches[0][:2]
    dirty = [dict(s, xhat_traj=s["xhat_traj"].clone()) for s in clean]
    dirty[1]["xhat_traj"][0, 200, 0] = float("nan")  # atom 0 (N of ALA) in frame 200: psi
    _, _, d0 = _run(tmp_path / "clean", [clean], xyz=ref)
    _, smp, d1 = _run(tmp_path / "dirty", [dirty], xyz=ref)
    a, b = np.load(d0 / "1.npz"), np.load(d1 / "1.npz")
    assert int(b["nonfinite_frames"].item()) == 1 and int(b["unassigned_frames"].item()) == 1 and int(a["unassigned_frames"].item()) == 0
    assert a["transition_counts"].sum() - b["transition_counts"].sum() == 2  # the pairs (198, 200) and (200, 202)
    assert abs(b["metastable_probs"].sum() - 1) < 1e-14 and not np.array_equal(a["metastable_probs"], b["metastable_probs"])
    assert tree(str(d0))["0.npz"] == tree(str(d1))["0.npz"]
    j = np.load(d1 / "joined.npz")
    assert int(j["nonfinite_frames"].item()) == 1 and int(j["unassigned_frames"].item()) == 1 and np.isfinite(list(smp.fabric.logged[-1].values())[0])


@pytest.mark.parametrize("case", ["none", "short_tica", "short_msm", "nan"])
def test_meter_without_a_usable_reference_writes_the_note_only(tmp_path, case):
    mol = dipeptide()
    ref, batches = mc.meter_fixture(mol, torch.device("cpu"))
    xyz = {"none": None, "short_tica": ref[:5], "short_msm": ref[:40], "nan": ref.clone()}[case]
    if case == "nan":
        xyz[900, 3, 1] = float("nan")
    cb, smp, d = _run(tmp_path, batches[:1], xyz=xyz, **({"msm_lag": 40} if case == "short_msm" else {}))
    assert os.listdir(d) == ["model.json"]
    info = json.load(open(d / "model.json"))
    want = {"none": "no reference frames", "short_tica": "no lag pair", "short_msm": "lag of the Markov state model", "nan": "non-finite feature"}[case]
    assert info["k_eff"] is None and want in info["note"] and smp.fabric.logged == [{}] and cb.meters["m"].compute() == {}


def test_config_names_the_callback_and_the_default_run_does_not(tmp_path):
    from jamun_amd import callbacks, cmdline, config

    cfg_dir = os.path.join(ROOT, "jamun_amd", "hydra_config", "callbacks", "sampler")
    assert "msm" not in open(os.path.join(cfg_dir, "default.yaml")).read()
    base = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=c"]
    assert "msm" not in cmdline.compose(base)["callbacks"]
    entry = cmdline.compose(base + ["callbacks=[sampler/default,sampler/msm]"])["callbacks"]["msm"]
    assert entry["_target_"] == "jamun.callbacks.sampler.MSMMetricsCallback"
    assert (entry["k"], entry["max_iter"], entry["seed"], entry["msm_lag"], entry["n_metastable"], entry["traj_lag"], entry["n_steps"], entry["lag"]) == (
        100, 100, 137, 1000, 10, 10, 50, 1000)
    cb = config.instantiate({k: v for k, v in entry.items() if k != "datasets"}, datasets=[CaseDataset(dipeptide(), "m")])
    assert isinstance(cb, callbacks.MSMMetricsCallback)
    meter = cb.meters["m"]
    assert (meter.k, meter.seed, meter.msm_lag, meter.n_metastable, meter.traj_lag, meter.n_steps, meter.lag, meter.width) == (100, 137, 1000, 10, 10, 50, 1000, 4)
    ds = CaseDataset(dipeptide(), "m")
    for kw in (dict(k=0), dict(msm_lag=0), dict(n_metastable=2.5), dict(traj_lag=0), dict(n_steps=0), dict(device="gpu")):
        with pytest.raises(ValueError):
            msm.MSMMetrics(ds, output_dir=str(tmp_path), **kw)
    ref, batches = mc.meter_fixture(dipeptide(), torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"MSMMetrics\(device='device'\) needs float32 sample tensors on a GPU"):
        _run(tmp_path, batches[:1], xyz=ref, device="device")


def test_the_fixture_is_stable_and_the_tolerances_are_ten_times_what_it_shows(tmp_path):
    """Every projected value moved by +-`_tica_cases.METER_TOLERANCE["tic01"]` (what the device path may differ by), 16 draws: no microstate
    label and no integer output changes (`_msm_cases.measure_stability` asserts it), and the float outputs move by `_msm_cases.OBSERVED`
    (within a factor 2)."""
    from jamun_amd.callbacks import MSMMetricsCallback

    mol = dipeptide()
    ref, batches = mc.meter_fixture(mol, torch.device("cpu"))
    features = {}
    count = [0]

    def run(shift):
        labels = []

        class Shifted(MSMMetricsCallback):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                for meter in self.meters.values():
                    inner_features, inner_project, inner_labels = meter._features, meter._project, meter._labels_of

                    def cached(frames, inner=inner_features):  # (the features do not depend on the shift: computed once per trajectory)
                        key = (tuple(frames.shape), float(np.asarray(frames[0, 0, 0])), float(np.asarray(frames[-1, -1, -1])))
                        if key not in features:
                            features[key] = inner(frames)
                        return features[key]

                    def project(x, inner=inner_project):
                        proj, bad = inner(x)
                        return shift(proj), bad

                    def labels_of(proj, inner=inner_labels):
                        labels.append(np.array(inner(proj)))
                        return labels[-1]

                    meter._features, meter._project, meter._labels_of = cached, project, labels_of

        count[0] += 1
        cb, _, d = _run(tmp_path / str(count[0]), batches, xyz=ref, callback=Shifted)
        model = np.load(d / "model.npz")
        assert json.load(open(d / "model.json"))["note"] is None
        ref_proj = cb.meters["m"]._project(cb.meters["m"]._features(ref))[0]  # (shifted again by the next draw of the same generator: another shift of the same size)
        return mc.meter_outputs(d), labels + [msm.assign_centers_host(ref_proj, model["centers"])[0]]

    seen = mc.measure_stability(run)
    print("largest changes:", seen)
    assert set(seen) == set(mc.OBSERVED)
    for k, v in seen.items():
        assert 0.5 * mc.OBSERVED[k] <= v <= 2.0 * mc.OBSERVED[k], (k, v, mc.OBSERVED[k])
        assert mc.TOLERANCE[k] == 10.0 * mc.OBSERVED[k]
