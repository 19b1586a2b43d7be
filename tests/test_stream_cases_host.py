"""The premises of test_gpu_streams.py, on the CPU: the case tables of _stream_cases.py build; under the host paths and the oracle the
stale and the true inputs of every case give results that are not equal, output by output, so a call that read its input before the
producer wrote it could not pass; the stale inputs are finite, of the shape and type of the true ones, and every index among them is in
range (a misordered read gives a wrong answer, never a fault); and the samplers select the paths the GPU file asserts through
``jamun_sampler_stats``."""
import numpy as np
import pytest
import torch

import _select_cases as sel
import _stream_cases as stc


def _assert_stale_is_visible(case):
    true, stale = case.inputs("true"), case.inputs("stale")
    assert sorted(true) == sorted(stale)
    for k in true:
        a, b = true[k], stale[k]
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous(), (case, k)
        assert not torch.equal(a, b), (case, k)
        if a.is_floating_point() and case.name != "hist2d_pairs_then_js_divergence":  # (the angle table holds NaN and inf on purpose: skipped frames)
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), (case, k)
    if not true:
        return
    want, other = case.host(true), case.host(stale)
    assert len(want) == len(other) >= 1
    for i, (a, b) in enumerate(zip(want, other)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.size > 0, (case, i)
        assert not np.array_equal(a, b, equal_nan=True), (case, i)


@pytest.mark.parametrize("case", stc.OPERATOR_CASES + stc.ANALYSIS_CASES, ids=repr)
def test_stale_inputs_change_the_result_of_every_operator_and_analysis_case(case):
    _assert_stale_is_visible(case)
    for v in case.fixed().values():
        assert torch.is_tensor(v) and v.is_contiguous(), case


@pytest.mark.parametrize("sampler", list(stc.SAMPLERS))
def test_stale_inputs_change_the_result_of_every_sampler_case(sampler):
    for op in stc.SAMPLER_OPS:
        _assert_stale_is_visible(stc.sampler_case(sampler, op))


def test_the_case_tables_cover_what_the_gpu_file_runs():
    assert len(stc.SAMPLER_CASES) == len(stc.SAMPLERS) * len(stc.SAMPLER_OPS) == 42
    names = [c.name for c in stc.OPERATOR_CASES + stc.ANALYSIS_CASES]
    assert len(set(names)) == len(names)
    for entry in ("mean_center", "radius_graph", "scatter_mean", "edge_geometry", "node_linear", "philox_normal", "baoab_pre_post", "aboba_a_b",
                  "encode_pdb_models", "encode_dcd_frames", "superpose_then_internal_coords", "hist2d_pairs_then_js_divergence", "validity_counts",
                  "lagged_moments", "project_frames", "autocov_sums", "assign_centers", "cluster_sums", "transition_counts", "label_counts"):
        assert entry in names
    assert stc.CONTROLS["sampler"] in stc.SAMPLER_CASES
    assert stc.case_by_name(stc.OPERATOR_CASES, stc.CONTROLS["operators"]).inputs("true")
    assert stc.case_by_name(stc.ANALYSIS_CASES, stc.CONTROLS["analysis"]).inputs("true")


def test_stale_labels_and_tables_stay_in_the_range_the_kernels_guard():
    """Labels out of range are part of the true case too (the kernels skip them); the tables that index memory are fixed, not stale."""
    for which in ("true", "stale"):
        lab = stc._labels(which)
        assert lab.dtype == torch.int32 and lab.shape == (stc.MSM_T,)
    assert (np.diff(stc.MSM_BOUNDS) >= 0).all() and stc.MSM_BOUNDS[0] == 0 and stc.MSM_BOUNDS[-1] == stc.MSM_T
    assert stc.HIST_PAIRS.max() < stc.HIST_W and stc.HIST_CUTS[-1] == stc.HIST_T
    _, index = stc._rigid()
    assert index.shape == (stc.IC_F, 4) and index.max() < stc._rigid()[0].shape[1]


def test_the_walk_keeps_trajectory_score_and_xhat_frames():
    import _switch_cases as sc

    n_y, n_baoab, n_aboba = sc.reference_frame_counts(stc.WALK_STEPS, stc.WALK_SAVE_EVERY, stc.WALK_BURN_IN)
    assert n_y >= 2 and n_baoab >= 2 and n_aboba >= 2


@pytest.mark.parametrize("name", list(stc.SAMPLERS))
def test_each_sampler_selects_the_path_it_is_there_for(name):
    arch, _, tuning, want = stc.SAMPLERS[name]
    st = sel.as_stats(sel.select(list(stc.sampler_molecules(name)), arch, tuning))
    assert want(st), (name, st)
