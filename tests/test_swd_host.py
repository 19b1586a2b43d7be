"""CPU tests of jamun_amd/swd.py: the host specification of the sliced Wasserstein distance (projection, order image, segment sort, merge,
quantile integral) against independent loops and a brute force, the constants and symbols of the device path, and the meter on the host
path against `sliced_wasserstein_host` on the concatenated frames."""
import os
import re

import numpy as np
import pytest
import torch

import _swd_cases as sc
from _frames_common import CaseDataset, meter_run, tree
from _traj_molecules import dipeptide
from jamun_amd import native, swd
from jamun_amd.features import internal_coords_host
from jamun_amd.ramachandran import sample_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- W2^2 -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", sc.W2SQ_SHAPES, ids=[f"{n}x{m}" for n, m in sc.W2SQ_SHAPES])
def test_w2sq_equals_the_brute_force(n, m):
    u, v = sc.sorted_columns(5, n, seed=n), sc.sorted_columns(5, m, seed=1000 + m)
    got, want = swd.w2sq_sorted_host(u, v), sc.brute_w2sq(u, v)
    assert got.dtype == np.float64 and got.shape == (5,)
    rel = np.abs(got - want) / want
    print(f"({n}, {m}): worst relative difference {rel.max():.2e}, bound {sc.w2sq_bound(n, m):.2e}")
    assert (rel <= sc.w2sq_bound(n, m)).all()


@pytest.mark.parametrize("n", [1, 5, 257])
def test_w2sq_of_equal_clouds_is_zero_and_of_a_shift_is_its_square(n):
    u = sc.sorted_columns(3, n, seed=7)
    assert (swd.w2sq_sorted_host(u, u) == 0.0).all()
    c = np.float32(0.75)  # (u + c is rounded; the distance is taken between the rounded clouds, whose differences are what is squared)
    v = (u + c).astype(np.float32)
    want = np.mean((v.astype(np.float64) - u.astype(np.float64)) ** 2, axis=1)
    got = swd.w2sq_sorted_host(v, u)
    assert (np.abs(got - want) <= sc.w2sq_bound(n, n) * want).all()
    exact = np.arange(n, dtype=np.float32)[None, :]  # whole numbers: the shift is exact, so the value is c^2
    assert (np.abs(swd.w2sq_sorted_host(exact + c, exact) - float(c) ** 2) <= sc.w2sq_bound(n, n) * float(c) ** 2).all()


def test_w2sq_with_a_non_finite_key_is_non_finite_in_that_row_only():
    u, v = sc.sorted_columns(3, 6, seed=1), sc.sorted_columns(3, 4, seed=2)
    clean = swd.w2sq_sorted_host(u, v)
    u[1, -1] = np.nan
    got = swd.w2sq_sorted_host(u, v)
    assert np.isnan(got[1]) and got[0] == clean[0] and got[2] == clean[2]
    with pytest.raises(ValueError):
        swd.w2sq_sorted_host(u[:2], v)


# ---- projection, directions ------------------------------------------------------------------------------------------------------------------

def test_project_host_equals_a_double_loop_bit_for_bit():
    rng = np.random.RandomState(0)
    x, proj = rng.randn(9, 6).astype(np.float32), rng.randn(6, 3).astype(np.float32)
    want = np.empty((3, 9), dtype=np.float32)
    for l in range(3):
        for t in range(9):
            acc = 0.0
            for j in range(6):
                acc = acc + float(x[t, j]) * float(proj[j, l])
            want[l, t] = np.float32(acc)
    got = swd.project_host(x, proj)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        swd.project_host(x.astype(np.float64), proj)


def test_projections_are_unit_columns_reproducible_and_pots_draw():
    p = swd.projections(8, 20, seed=3)
    assert p.dtype == np.float32 and p.shape == (8, 20)
    norms = np.sqrt((p.astype(np.float64) ** 2).sum(axis=0))
    assert (np.abs(norms - 1.0) <= 2.0 ** -23).all()  # (within one ulp of float32)
    assert np.array_equal(p, swd.projections(8, 20, seed=3)) and not np.array_equal(p, swd.projections(8, 20, seed=4))
    raw = np.random.RandomState(3).randn(8, 20)
    assert np.array_equal(p, (raw / np.sqrt((raw ** 2).sum(0, keepdims=True))).astype(np.float32))
    for bad in (dict(d=0), dict(d=4, n_projections=0), dict(d=2.5)):
        with pytest.raises(ValueError):
            swd.projections(**bad)


def test_descriptor_rows_is_the_permutation_to_the_references_order():
    rows = swd.descriptor_rows(2, 3)
    assert sorted(rows.tolist()) == list(range(10))
    # interleaved: cos phi0, sin phi0, cos phi1, sin phi1, cos psi0, sin psi0, ...; the reference: cos phi (2), sin phi (2), cos psi (3), sin psi (3)
    assert rows.tolist() == [0, 2, 1, 3, 4, 7, 5, 8, 6, 9]
    assert swd.descriptor_rows(1, 1).tolist() == [0, 1, 2, 3] and swd.descriptor_rows(0, 0).shape == (0,)


# ---- order, sort, merge ----------------------------------------------------------------------------------------------------------------------

def test_order_image_is_monotone_on_the_table_of_special_values():
    keys = sc.special_keys()
    image = swd.order_image(keys)
    assert image.dtype == np.uint32 and (np.diff(image.astype(np.int64)) > 0).all()
    assert (swd.order_image(sc.nan_keys()) == 0xFFFFFFFF).all() and image.max() < 0xFFFFFFFF
    back = swd.keys_of_image(image)
    assert np.array_equal(back.view(np.uint32), keys.view(np.uint32))
    assert (swd.keys_of_image(swd.order_image(sc.nan_keys())).view(np.uint32) == 0x7FC00000).all()
    finite = np.sort(np.random.RandomState(0).randn(1000).astype(np.float32))
    assert (np.diff(swd.order_image(finite).astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("kind", ["random", "sorted", "reversed", "equal", "ties", "special"])
def test_sort_segments_and_merge_equal_a_sort_of_the_image(kind):
    keys = sc.key_data(kind, 3, 41, seed=5)
    cuts = [1, 2, 17, 40]
    got = swd.sort_segments_host(keys, cuts)
    assert got.dtype == np.float32 and got.shape == keys.shape
    start = 0
    for c in cuts:
        assert np.array_equal(swd.order_image(got[:, start:c]), np.sort(swd.order_image(keys[:, start:c]), axis=1))
        start = c
    assert np.array_equal(got[:, 40:].view(np.uint32), keys[:, 40:].view(np.uint32))  # behind the last cut: as it was
    a, b = swd.sort_segments_host(keys[:, :17], [17]), swd.sort_segments_host(keys[:, 17:], [24])
    merged = swd.merge_sorted_host(a, b)
    assert np.array_equal(swd.order_image(merged), np.sort(swd.order_image(keys), axis=1))
    assert np.array_equal(merged.view(np.uint32), swd.sort_segments_host(keys, [41]).view(np.uint32))
    nan = np.isnan(merged)
    assert (merged.view(np.uint32)[nan] == 0x7FC00000).all() and (np.diff(nan.astype(int), axis=1) >= 0).all()  # NaN last, canonical


def test_sort_refuses_bad_cuts_and_shapes():
    keys = sc.key_data("random", 2, 10)
    for cuts in ([], [0], [11], [5, 5], [6, 3], list(range(1, 66))):
        with pytest.raises(ValueError):
            swd.sort_segments_host(np.tile(keys, (1, 7)) if len(cuts) > 64 else keys, cuts)
    with pytest.raises(ValueError):
        swd.merge_sorted_host(keys, keys[:1])
    with pytest.raises(ValueError):
        swd.sort_segments_host(keys.astype(np.float64), [10])


def test_sliced_wasserstein_host_composes_the_parts():
    rng = np.random.RandomState(1)
    x, y = rng.randn(50, 4).astype(np.float32), (rng.randn(31, 4) + 0.5).astype(np.float32)
    proj = swd.projections(4, 20, 0)
    d = swd.sliced_wasserstein_host(x, y, proj)
    per = [sc.brute_w2sq(np.sort(x @ proj[:, l:l + 1], axis=0).T.astype(np.float32), np.sort(y @ proj[:, l:l + 1], axis=0).T.astype(np.float32))[0] for l in range(20)]
    assert abs(d - np.sqrt(np.mean(per))) <= 1e-6 * d and swd.sliced_wasserstein_host(x, x, proj) == 0.0  # (x @ proj in fp32: close, not equal)


# ---- the device path's constants, symbols and refusals that need no GPU -----------------------------------------------------------------------

def test_constants_mirror_the_kernels_and_the_symbols_are_bound():
    from jamun_amd import _lib
    from jamun_amd.csrc import build

    hdr = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_internal.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))
    assert (native.SWD_TILE, native.SWD_MAX_WIDTH, native.SWD_MAX_PROJ) == (macro("JAMUN_SWD_TILE"), macro("JAMUN_SWD_MAX_WIDTH"), macro("JAMUN_SWD_MAX_PROJ"))
    assert (native.SWD_MAX_WIDTH, native.SWD_MAX_PROJ) == (128, 64) and native.SWD_TILE * 4 <= 65536
    assert "jamun_swd.hip" in build.SOURCES
    lib = _lib.load()
    for name in ("jamun_swd_project", "jamun_swd_sort_work", "jamun_swd_sort_segments", "jamun_swd_merge", "jamun_swd_w2sq_work", "jamun_swd_w2sq"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_wrappers_refuse_on_the_host_before_a_gpu_is_needed():
    x, keys = torch.zeros(5, 4), torch.zeros(3, 5)
    for call in (lambda: native.swd_project(torch.zeros(0, 4), np.zeros((4, 2), np.float32)),
                 lambda: native.swd_project(x, np.zeros((3, 2), np.float32)),
                 lambda: native.swd_project(x, np.zeros((4, 65), np.float32)),
                 lambda: native.swd_project(torch.zeros(5, 129), np.zeros((129, 2), np.float32)),
                 lambda: native.swd_project(x, np.zeros((4, 2), np.float64)),
                 lambda: native.swd_sort_segments(keys, [0]),
                 lambda: native.swd_sort_segments(keys, [3, 3]),
                 lambda: native.swd_sort_segments(keys, [6]),
                 lambda: native.swd_sort_segments(torch.zeros(65, 5), [5]),
                 lambda: native.swd_sort_segments(torch.zeros(3, 0), [1]),
                 lambda: native.swd_merge(keys, torch.zeros(2, 5)),
                 lambda: native.swd_merge(keys, torch.zeros(3, 0)),
                 lambda: native.swd_w2sq(keys, torch.zeros(2, 5)),
                 lambda: native.swd_w2sq(torch.zeros(5), keys)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: native.swd_project(x, np.zeros((4, 2), np.float32)), lambda: native.swd_sort_segments(keys, [5]),
                 lambda: native.swd_merge(keys, keys), lambda: native.swd_w2sq(keys, keys)):
        with pytest.raises(RuntimeError, match="on the GPU"):  # (CPU tensors: refused before the library is asked for a device)
            call()


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    """Every refusal of the six entries is raised before any HIP call: null pointers stand for the device buffers throughout."""
    import ctypes as C

    from jamun_amd import _lib

    lib = _lib.load()
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    cuts = (C.c_int32 * 2)(3, 8)
    bad_cuts = (C.c_int32 * 2)(3, 3)
    out = C.c_int64(-1)
    cases = [
        ("width", lambda: lib.jamun_swd_project(p, 4, 8, 0, p, 2, p, 16, None)),
        ("width", lambda: lib.jamun_swd_project(p, 129, 8, 129, p, 2, p, 16, None)),
        ("n_proj", lambda: lib.jamun_swd_project(p, 4, 8, 4, p, 65, p, 8 * 65, None)),
        ("n_frames", lambda: lib.jamun_swd_project(p, 4, 0, 4, p, 2, p, 16, None)),
        ("row_stride", lambda: lib.jamun_swd_project(p, 3, 8, 4, p, 2, p, 16, None)),
        ("out_capacity", lambda: lib.jamun_swd_project(p, 4, 8, 4, p, 2, p, 15, None)),
        ("null", lambda: lib.jamun_swd_project(None, 4, 8, 4, p, 2, p, 16, None)),
        ("null", lambda: lib.jamun_swd_project(p, 4, 8, 4, p, 2, None, 16, None)),
        ("null", lambda: lib.jamun_swd_sort_work(8, 2, cuts, 2, None)),
        ("cuts", lambda: lib.jamun_swd_sort_work(8, 2, bad_cuts, 2, C.byref(out))),
        ("cuts", lambda: lib.jamun_swd_sort_work(7, 2, cuts, 2, C.byref(out))),
        ("n_cuts", lambda: lib.jamun_swd_sort_work(8, 2, cuts, 0, C.byref(out))),
        ("n_cuts", lambda: lib.jamun_swd_sort_segments(p, 8, 2, cuts, 65, p, 16, None, 0, None)),
        ("null", lambda: lib.jamun_swd_sort_segments(p, 8, 2, None, 2, p, 16, None, 0, None)),
        ("n_proj", lambda: lib.jamun_swd_sort_segments(p, 8, 0, cuts, 2, p, 16, None, 0, None)),
        ("n_frames", lambda: lib.jamun_swd_sort_segments(p, 0, 2, cuts, 2, p, 16, None, 0, None)),
        ("out_capacity", lambda: lib.jamun_swd_sort_segments(p, 8, 2, cuts, 2, p, 15, None, 0, None)),
        ("null", lambda: lib.jamun_swd_sort_segments(None, 8, 2, cuts, 2, p, 16, None, 0, None)),
        ("null", lambda: lib.jamun_swd_sort_segments(p, 8, 2, cuts, 2, None, 16, None, 0, None)),
        ("n 0", lambda: lib.jamun_swd_merge(p, 4, 0, p, 4, 4, 2, p, 16, None)),
        ("m 0", lambda: lib.jamun_swd_merge(p, 4, 4, p, 4, 0, 2, p, 16, None)),
        ("n_proj", lambda: lib.jamun_swd_merge(p, 4, 4, p, 4, 4, 65, p, 8 * 65, None)),
        ("row strides", lambda: lib.jamun_swd_merge(p, 3, 4, p, 4, 4, 2, p, 16, None)),
        ("31 bits", lambda: lib.jamun_swd_merge(p, 2 ** 31 - 1, 2 ** 31 - 1, p, 4, 4, 2, p, 2 ** 40, None)),
        ("out_capacity", lambda: lib.jamun_swd_merge(p, 4, 4, p, 4, 4, 2, p, 15, None)),
        ("null", lambda: lib.jamun_swd_merge(p, 4, 4, None, 4, 4, 2, p, 16, None)),
        ("null", lambda: lib.jamun_swd_w2sq_work(4, 4, 2, None)),
        ("m 0", lambda: lib.jamun_swd_w2sq_work(4, 0, 2, C.byref(out))),
        ("n_proj", lambda: lib.jamun_swd_w2sq(p, 4, 4, p, 4, 4, 0, p, p, 64, None)),
        ("row strides", lambda: lib.jamun_swd_w2sq(p, 4, 4, p, 3, 4, 2, p, p, 64, None)),
        ("work_capacity", lambda: lib.jamun_swd_w2sq(p, 4, 4, p, 4, 4, 2, p, p, 1, None)),
        ("null", lambda: lib.jamun_swd_w2sq(p, 4, 4, p, 4, 4, 2, None, p, 64, None)),
        ("null", lambda: lib.jamun_swd_w2sq(p, 4, 4, p, 4, 4, 2, p, None, 64, None)),
    ]
    for want, call in cases:
        assert call() != 0, want
        assert want in lib.jamun_last_error().decode(), (want, lib.jamun_last_error())
    assert out.value == -1 and host.raw == b"\0" * 64
    assert lib.jamun_swd_sort_work(8, 2, cuts, 2, C.byref(out)) == 0 and out.value == 0  # (no segment longer than a tile: no workspace)
    long_cut = (C.c_int32 * 1)(native.SWD_TILE + 1)
    assert lib.jamun_swd_sort_work(native.SWD_TILE + 1, 3, long_cut, 1, C.byref(out)) == 0 and out.value == 3 * (native.SWD_TILE + 1)
    assert lib.jamun_swd_w2sq_work(257, 100, 3, C.byref(out)) == 0 and out.value == 3 * 2


# ---- the meter on the host path ------------------------------------------------------------------------------------------------------------------

def _run(root, batches, xyz=None, **kw):
    from jamun_amd.callbacks import SlicedWassersteinMetricsCallback

    cb, smp = meter_run(SlicedWassersteinMetricsCallback, root, dipeptide(), batches, torch.device("cpu"), xyz=xyz, **kw)
    return cb, smp, root / "m" / "sliced_wasserstein"


def _descriptors(meter, frames) -> np.ndarray:
    return internal_coords_host(frames, meter.index, cossin=True).astype(np.float32)


def test_meter_on_the_host_path_equals_the_specification_at_every_cut(tmp_path):
    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, torch.device("cpu"))
    cb, smp, d = _run(tmp_path, batches, xyz=ref)
    meter = cb.meters["m"]
    assert sorted(os.listdir(d)) == ["0.npz", "1.npz", "joined.npz", "projections.npz"]
    p = np.load(d / "projections.npz")
    assert np.array_equal(p["projections"], swd.projections(4, 20, 0)) and int(p["seed"].item()) == 0 and p["pairing"].item() == "reference"
    assert p["torsion_labels"].tolist() == meter.torsion_labels and len(meter.torsion_labels) == 2 and p["note"].item() == ""
    assert int(p["reference_frames"].item()) == sc.REFERENCE_T and p["descriptor_rows"].tolist() == [0, 1, 2, 3]
    proj = p["projections"][p["descriptor_rows"]]
    x_ref = _descriptors(meter, ref.numpy())
    xs = [_descriptors(meter, s["xhat_traj"].permute(1, 0, 2).numpy()) for s in batches[0]]
    T = sc.CHAIN_T
    for i, x in enumerate(xs):
        z = np.load(d / f"{i}.npz")
        assert sorted(z.files) == ["nonfinite", "num_samples", "w2sq_per_projection", "ws_distance"]
        assert z["num_samples"].tolist() == sample_counts(T) == [100, 200, 250] and z["w2sq_per_projection"].shape == (3, 20)
        assert (z["nonfinite"] == 0).all() and z["ws_distance"].dtype == np.float64
        for k, v in zip(z["num_samples"], z["ws_distance"]):
            assert v == swd.sliced_wasserstein_host(x[:k], x_ref, proj) and 0.0 < v < 2.0
    j = np.load(d / "joined.npz")
    cat = np.concatenate(xs)
    assert j["num_samples"].tolist() == [100, 200, 400, 500]  # (400 falls inside the second chain)
    for k, v in zip(j["num_samples"], j["ws_distance"]):
        assert v == swd.sliced_wasserstein_host(cat[:k], x_ref, proj)
    assert smp.fabric.logged == [{"m/ws_distance/pred_traj_joined": float(j["ws_distance"][-1])}]
    assert meter.joined_sorted.shape == (20, 2 * T) and meter.joined_sorted.dtype == np.float32  # 4 L bytes per joined frame
    _run(tmp_path / "again", batches, xyz=ref)
    assert tree(str(d)) == tree(str(tmp_path / "again" / "m" / "sliced_wasserstein"))


def test_meter_merges_the_reference_chunks(tmp_path, monkeypatch):
    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, torch.device("cpu"))
    _, _, whole = _run(tmp_path / "whole", batches, xyz=ref)
    monkeypatch.setattr(swd.SlicedWassersteinMetrics, "REFERENCE_CHUNK", 256)
    _, _, parts = _run(tmp_path / "parts", batches, reference=ref.numpy())
    assert tree(str(whole)) == tree(str(parts))  # (a sorted column is unique as bits)


def test_meter_reports_nan_for_a_prefix_with_a_non_finite_frame(tmp_path):
    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, torch.device("cpu"))
    dirty = [dict(s, xhat_traj=s["xhat_traj"].clone()) for s in batches[0]]
    dirty[0]["xhat_traj"][0, 150, 0] = float("nan")  # atom 0 (N of ALA) in frame 150 of the first chain: psi
    _, smp, d0 = _run(tmp_path / "clean", batches, xyz=ref)
    _, smp, d1 = _run(tmp_path / "dirty", [dirty], xyz=ref)
    a, b = np.load(d0 / "0.npz"), np.load(d1 / "0.npz")
    assert b["nonfinite"].tolist() == [0, 1, 1] and b["ws_distance"][0] == a["ws_distance"][0] and np.isnan(b["ws_distance"][1:]).all()
    assert np.isnan(b["w2sq_per_projection"][1:]).any() and tree(str(d0))["1.npz"] == tree(str(d1))["1.npz"]
    j, j0 = np.load(d1 / "joined.npz"), np.load(d0 / "joined.npz")
    assert j["nonfinite"].tolist() == [0, 1, 1, 1] and j["ws_distance"][0] == j0["ws_distance"][0] and np.isnan(j["ws_distance"][1:]).all()
    assert np.isnan(smp.fabric.logged[-1]["m/ws_distance/pred_traj_joined"])


def test_meter_without_reference_frames_writes_the_note_only(tmp_path):
    ref, batches = sc.meter_fixture(dipeptide(), torch.device("cpu"))
    cb, smp, d = _run(tmp_path, batches)
    assert os.listdir(d) == ["projections.npz"] and "no reference frames" in np.load(d / "projections.npz")["note"].item()
    assert smp.fabric.logged == [{}] and cb.meters["m"].compute() == {}


def test_meter_arguments_the_device_message_and_the_config(tmp_path):
    from jamun_amd import callbacks, cmdline, config

    ds = CaseDataset(dipeptide(), "m")
    for kw in (dict(n_projections=0), dict(n_projections=2.5), dict(seed=-1), dict(pairing="other"), dict(device="gpu")):
        with pytest.raises(ValueError):
            swd.SlicedWassersteinMetrics(ds, output_dir=str(tmp_path), **kw)
    with pytest.raises(ValueError, match="no molecule"):
        swd.SlicedWassersteinMetrics(CaseDataset(None, "m"))
    ref, batches = sc.meter_fixture(dipeptide(), torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"SlicedWassersteinMetrics\(device='device'\) needs float32 sample tensors on a GPU"):
        _run(tmp_path, batches, xyz=ref, device="device")
    cfg_dir = os.path.join(ROOT, "jamun_amd", "hydra_config", "callbacks", "sampler")
    assert "wasserstein" not in open(os.path.join(cfg_dir, "default.yaml")).read()
    base = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=c"]
    assert "sliced_wasserstein" not in cmdline.compose(base)["callbacks"]
    entry = cmdline.compose(base + ["callbacks=[sampler/default,sampler/sliced_wasserstein]"])["callbacks"]["sliced_wasserstein"]
    assert entry["_target_"] == "jamun.callbacks.sampler.SlicedWassersteinMetricsCallback"
    assert (entry["n_projections"], entry["seed"], entry["pairing"]) == (20, 0, "reference")
    cb = config.instantiate({k: v for k, v in entry.items() if k != "datasets"}, datasets=[ds])
    assert isinstance(cb, callbacks.SlicedWassersteinMetricsCallback)
    meter = cb.meters["m"]
    assert (meter.n_projections, meter.seed, meter.width, meter.mode) == (20, 0, 4, "auto")


def test_the_meter_tolerance_is_ten_times_what_the_fixture_shows():
    """`_swd_cases.TOLERANCE` against a fresh measurement (within a factor 2: the draws of the signs are the same)."""
    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, torch.device("cpu"))
    meter = swd.SlicedWassersteinMetrics(CaseDataset(mol, "m"), device="host")
    seen = sc.measure_sensitivity(_descriptors(meter, ref.numpy()), [_descriptors(meter, s["xhat_traj"].permute(1, 0, 2).numpy()) for s in batches[0]],
                                  meter.proj_rows, sample_counts)
    print(f"largest change of a ws_distance: {seen:.3e} (recorded {sc.OBSERVED:.3e})")
    assert 0.5 * sc.OBSERVED <= seen <= 2.0 * sc.OBSERVED and sc.TOLERANCE == 10.0 * sc.OBSERVED
