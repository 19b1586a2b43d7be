"""GPU tests of jamun_swd.hip (projection, segment sort, merge, quantile integral), of their refusals, of their stream contract and of
the sliced Wasserstein meter on the device path.  The expected values are the host specification's (jamun_amd/swd.py, pinned against loops
and a brute force in test_swd_host.py): keys and sorted columns are compared as bits, W2^2 within (n + m) 2^-52 relative."""
import os

import numpy as np
import pytest
import torch

import _swd_cases as sc
from _frames_common import _dev, guarded, intact, meter_run
from _traj_molecules import dipeptide
from jamun_amd import native, swd

pytestmark = pytest.mark.gpu

TILE = native.SWD_TILE


def _bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _up(a, dev):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)


# ---- projection ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,L", [(1, 1), (4, 20), (128, 64), (4, 64), (128, 1)])
def test_project_equals_the_specification_bit_for_bit(W, L):
    dev = _dev()
    for T in (1, 63, 65, TILE + 1):
        rng = np.random.RandomState(W * 1000 + L + T)
        x, proj = rng.randn(T, W).astype(np.float32), rng.randn(W, L).astype(np.float32)
        got = native.swd_project(_up(x, dev), proj)
        assert got.dtype == torch.float32 and tuple(got.shape) == (L, T) and got.is_contiguous()
        assert np.array_equal(_bits(got), _bits(swd.project_host(x, proj))), (W, L, T)


def test_project_reads_a_row_strided_view_and_passes_non_finite_rows_on():
    dev = _dev()
    rng = np.random.RandomState(3)
    wide = rng.randn(70, 11).astype(np.float32)
    wide[5, 2], wide[9, 0] = np.nan, np.inf
    wide[:, 4:] = np.nan  # (behind the 4 columns of the view: never read)
    proj = swd.projections(4, 20, 1)
    view = _up(wide, dev)[:, :4]
    assert view.stride() == (11, 1)
    big, out = guarded((20, 70), dev, torch.float32, -7.0)
    got = native.swd_project(view, _up(proj, dev), out=out)
    assert got is out and intact(big, -7.0)
    assert np.array_equal(_bits(got), _bits(swd.project_host(np.ascontiguousarray(wide[:, :4]), proj)))
    assert not np.isfinite(got.cpu().numpy()[:, [5, 9]]).any()


# ---- sort ------------------------------------------------------------------------------------------------------------------------------------

def _cuts_for(T: int):
    """1, a tile boundary - 1, the boundary, the boundary + 1, and T (those that lie within [1, T], ascending)."""
    return sorted({c for c in (1, TILE - 1, TILE, TILE + 1, 2 * TILE, T) if 1 <= c <= T})


@pytest.mark.parametrize("kind", ["random", "sorted", "reversed", "equal", "ties", "special"])
def test_sort_segments_gives_the_specifications_image(kind):
    dev = _dev()
    for T in (1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        keys = sc.key_data(kind, 3, T, seed=T)
        for cuts in ([T], _cuts_for(T)):
            got = native.swd_sort_segments(_up(keys, dev), cuts)
            want = swd.sort_segments_host(keys, cuts)
            assert np.array_equal(swd.order_image(got.cpu().numpy()), swd.order_image(want)), (kind, T, cuts)
            assert np.array_equal(_bits(got), _bits(want)), (kind, T, cuts)  # (unique as bits: NaN is the quiet NaN)


def test_sort_leaves_the_frames_behind_the_last_cut_and_the_input_and_takes_keys_as_out():
    dev = _dev()
    T = 2 * TILE + 9
    keys = sc.key_data("special", 2, T, seed=1)
    k = _up(keys, dev)
    big, out = guarded((2, T), dev, torch.float32, -7.0)
    for cuts in ([5, TILE + 3], [5, 2 * TILE + 2]):  # (no merge pass; one merge pass: the last step lands in `out` either way)
        got = native.swd_sort_segments(k, cuts, out=out)
        assert got is out and intact(big, -7.0) and np.array_equal(_bits(k), _bits(keys))
        assert np.array_equal(_bits(got), _bits(swd.sort_segments_host(keys, cuts))), cuts
        same = k.clone()
        assert native.swd_sort_segments(same, cuts, out=same) is same
        assert np.array_equal(_bits(same), _bits(swd.sort_segments_host(keys, cuts))), cuts


# ---- merge ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(1, 1), (1, TILE + 1), (TILE, TILE), (2 * TILE + 3, 7)])
@pytest.mark.parametrize("kind", ["random", "ties", "special"])
def test_merge_gives_the_specifications_image(n, m, kind):
    dev = _dev()
    a = swd.sort_segments_host(sc.key_data(kind, 3, n, seed=n), [n])
    b = swd.sort_segments_host(sc.key_data(kind, 3, m, seed=m + 1), [m])
    want = swd.merge_sorted_host(a, b)
    for x, y in ((a, b), (b, a)):
        got = native.swd_merge(_up(x, dev), _up(y, dev))
        assert tuple(got.shape) == (3, n + m) and np.array_equal(swd.order_image(got.cpu().numpy()), swd.order_image(want))
        assert np.array_equal(_bits(got), _bits(want))


def test_merge_reads_segments_of_a_sorted_array_in_place():
    dev = _dev()
    T = TILE + 300
    keys = sc.key_data("random", 4, T, seed=2)
    seg = native.swd_sort_segments(_up(keys, dev), [200, T])
    a, b = seg[:, :200], seg[:, 200:]
    assert a.stride() == (T, 1) and not b.is_contiguous()
    big, out = guarded((4, T), dev, torch.float32, -7.0)
    got = native.swd_merge(a, b, out=out)
    assert intact(big, -7.0) and np.array_equal(_bits(got), _bits(swd.sort_segments_host(keys, [T])))


# ---- W2^2 --------------------------------------------------------------------------------------------------------------------------------------

W2SQ_SHAPES = sc.W2SQ_SHAPES + [(3 * TILE + 5, 100), (100, 3 * TILE + 5)]


@pytest.mark.parametrize("n,m", W2SQ_SHAPES, ids=[f"{n}x{m}" for n, m in W2SQ_SHAPES])
def test_w2sq_is_within_the_bound_of_the_specification_and_the_same_in_two_runs(n, m):
    dev = _dev()
    u, v = sc.sorted_columns(5, n, seed=n), sc.sorted_columns(5, m, seed=1000 + m)
    want = swd.w2sq_sorted_host(u, v)
    ud, vd = _up(u, dev), _up(v, dev)
    got = native.swd_w2sq(ud, vd)
    again = native.swd_w2sq(ud, vd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,) and np.array_equal(_bits(got), _bits(again))
    rel = np.abs(got.cpu().numpy() - want) / want
    print(f"({n}, {m}): worst relative difference {rel.max():.2e}, bound {sc.w2sq_bound(n, m):.2e}")
    assert (rel <= sc.w2sq_bound(n, m)).all()
    assert (native.swd_w2sq(ud, ud).cpu().numpy() == 0.0).all()


def test_w2sq_with_a_nan_in_one_column_leaves_the_others_exact():
    dev = _dev()
    u, v = sc.sorted_columns(4, TILE + 7, seed=1), sc.sorted_columns(4, 300, seed=2)
    clean = native.swd_w2sq(_up(u, dev), _up(v, dev)).cpu().numpy()
    u[2, -1] = np.nan
    wide = np.full((4, TILE + 20), np.nan, dtype=np.float32)  # a row stride: nothing behind a row's keys is read
    wide[:, : TILE + 7] = u
    got = native.swd_w2sq(_up(wide, dev)[:, : TILE + 7], _up(v, dev)).cpu().numpy()
    assert np.isnan(got[2]) and np.array_equal(_bits(got[[0, 1, 3]]), _bits(clean[[0, 1, 3]]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_outputs_untouched():
    """The C entries on device buffers filled with a sentinel, and the wrappers with an ``out`` of a wrong kind: nothing is written."""
    import ctypes as C

    from jamun_amd import _lib

    lib = _lib.load()
    dev = _dev()
    x = torch.zeros((8, 4), device=dev)
    proj = torch.zeros((4, 2), device=dev)
    keys = torch.zeros((2, 8), device=dev)
    out = torch.full((64,), -7.0, device=dev)
    out64 = torch.full((8,), -7.0, dtype=torch.float64, device=dev)
    work = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
    cuts, bad_cuts, far_cuts = (C.c_int32 * 2)(3, 8), (C.c_int32 * 2)(3, 3), (C.c_int32 * 2)(3, 9)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    calls = [
        lambda: lib.jamun_swd_project(p(x), 4, 8, 129, p(proj), 2, p(out), 64, st),
        lambda: lib.jamun_swd_project(p(x), 4, 8, 4, p(proj), 65, p(out), 64, st),
        lambda: lib.jamun_swd_project(p(x), 4, 0, 4, p(proj), 2, p(out), 64, st),
        lambda: lib.jamun_swd_project(p(x), 3, 8, 4, p(proj), 2, p(out), 64, st),
        lambda: lib.jamun_swd_project(p(x), 4, 8, 4, p(proj), 2, p(out), 15, st),
        lambda: lib.jamun_swd_project(None, 4, 8, 4, p(proj), 2, p(out), 64, st),
        lambda: lib.jamun_swd_project(p(x), 4, 8, 4, None, 2, p(out), 64, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 2, bad_cuts, 2, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 2, far_cuts, 2, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 2, cuts, 0, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 2, None, 2, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 65, cuts, 2, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(p(keys), 8, 2, cuts, 2, p(out), 15, None, 0, st),
        lambda: lib.jamun_swd_sort_segments(None, 8, 2, cuts, 2, p(out), 64, None, 0, st),
        lambda: lib.jamun_swd_merge(p(keys), 8, 0, p(keys), 8, 8, 2, p(out), 64, st),
        lambda: lib.jamun_swd_merge(p(keys), 8, 8, p(keys), 7, 8, 2, p(out), 64, st),
        lambda: lib.jamun_swd_merge(p(keys), 8, 8, p(keys), 8, 8, 2, p(out), 31, st),
        lambda: lib.jamun_swd_merge(p(keys), 8, 8, None, 8, 8, 2, p(out), 64, st),
        lambda: lib.jamun_swd_w2sq(p(keys), 8, 8, p(keys), 8, 0, 2, p(out64), p(work), 64, st),
        lambda: lib.jamun_swd_w2sq(p(keys), 7, 8, p(keys), 8, 8, 2, p(out64), p(work), 64, st),
        lambda: lib.jamun_swd_w2sq(p(keys), 8, 8, p(keys), 8, 8, 2, p(out64), p(work), 1, st),
        lambda: lib.jamun_swd_w2sq(p(keys), 8, 8, p(keys), 8, 8, 2, p(out64), None, 64, st),
        lambda: lib.jamun_swd_w2sq(None, 8, 8, p(keys), 8, 8, 2, p(out64), p(work), 64, st),
    ]
    for i, call in enumerate(calls):
        assert call() != 0, i
    # a segment longer than a tile needs a workspace: without one, or with one that overlaps out, the sort is refused
    T = TILE + 1
    long_keys = torch.zeros((1, T), device=dev)
    long_out = torch.full((2 * T,), -7.0, device=dev)
    long_cut = (C.c_int32 * 1)(T)
    assert lib.jamun_swd_sort_segments(p(long_keys), T, 1, long_cut, 1, p(long_out), T, None, 0, st) != 0
    assert lib.jamun_swd_sort_segments(p(long_keys), T, 1, long_cut, 1, p(long_out), T, p(long_out) + 4 * (T - 1), T, st) != 0
    for call, kind in ((lambda: native.swd_project(x, proj, out=torch.zeros((2, 7), device=dev)), RuntimeError),
                       (lambda: native.swd_project(x, proj, out=out64[:0]), RuntimeError),
                       (lambda: native.swd_sort_segments(keys, [8], out=torch.zeros((2, 8), dtype=torch.float64, device=dev)), RuntimeError),
                       (lambda: native.swd_sort_segments(torch.zeros((2, 16), device=dev)[:, ::2], [8]), RuntimeError),
                       (lambda: native.swd_merge(keys, keys, out=out[:16].view(2, 8)), RuntimeError),
                       (lambda: native.swd_w2sq(keys, keys.double()), RuntimeError),
                       (lambda: native.swd_w2sq(keys, keys.cpu()), RuntimeError),
                       (lambda: native.swd_sort_segments(keys, [9]), ValueError)):
        with pytest.raises(kind):
            call()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (out64 == -7.0).all() and (work == -7.0).all() and (long_out == -7.0).all()


# ---- the stream contract --------------------------------------------------------------------------------------------------------------------------

STREAM_T = 3 * TILE + 5


def _stream_cases():
    """name -> (inputs(which) -> dict of arrays, run(bufs) -> outputs): the stale inputs differ from the true ones in every result."""
    proj = swd.projections(4, 20, 0)

    def rows(which):
        return np.random.RandomState(0 if which == "true" else 1).randn(STREAM_T, 4).astype(np.float32)

    def keys(which):
        return swd.project_host(rows(which), proj)

    def sorted_keys(which, n):
        return swd.sort_segments_host(keys(which)[:, :n], [n])

    return {
        "project": (lambda w: {"x": rows(w)}, lambda b: [native.swd_project(b["x"], proj)]),
        "sort_segments": (lambda w: {"keys": keys(w)}, lambda b: [native.swd_sort_segments(b["keys"], [100, TILE + 1, STREAM_T])]),
        "merge": (lambda w: {"a": sorted_keys(w, 2 * TILE + 3), "b": sorted_keys(w, 7)}, lambda b: [native.swd_merge(b["a"], b["b"])]),
        "w2sq": (lambda w: {"u": sorted_keys(w, STREAM_T), "v": sorted_keys(w, 100)}, lambda b: [native.swd_w2sq(b["u"], b["v"])]),
    }


@pytest.fixture(scope="module")
def side_stream():
    """A side stream the null stream overtakes, and busy work for it (the rule of test_gpu_streams.py: a side stream that shares the null
    stream's hardware queue runs in submission order with it, and there a launch on the wrong stream cannot be told from one on the right)."""
    dev = _dev()
    a = (torch.randn(4096, 4096, generator=torch.Generator().manual_seed(0)) / 64.0).to(dev)
    scratch = torch.empty_like(a)

    def busy(steps=40):
        for _ in range(steps):
            torch.mm(a, a, out=scratch)

    busy(1)
    torch.cuda.synchronize()
    for _ in range(16):
        side = torch.cuda.Stream(dev)
        flag = torch.zeros(1, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            busy(10)
            flag.fill_(1.0)
        seen = flag.clone()  # (on the null stream)
        torch.cuda.synchronize()
        if seen.item() == 0.0:
            return side, busy
    raise AssertionError("no side stream runs independently of the null stream: these tests would see nothing")


@pytest.mark.parametrize("name", ["project", "sort_segments", "merge", "w2sq"])
def test_entries_on_a_side_stream_run_behind_their_producer(side_stream, name):
    """Busy work, a producer that overwrites stale inputs in place, the call and a consumer on one side stream; only that stream is
    synchronised.  The result equals the serial one on the true inputs bit for bit, and differs from the one on the stale inputs."""
    dev = _dev()
    side, busy = side_stream
    inputs, run = _stream_cases()[name]
    true = {k: _up(v, dev) for k, v in inputs("true").items()}
    stale = {k: _up(v, dev) for k, v in inputs("stale").items()}
    torch.cuda.synchronize()
    want = [o.clone() for o in run(true)]
    wrong = [o.clone() for o in run(stale)]
    torch.cuda.synchronize()
    assert not any(torch.equal(a, b) for a, b in zip(want, wrong))  # (stale inputs show)
    bufs = {k: v.clone() for k, v in stale.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy()
        for k in bufs:
            bufs[k].copy_(true[k])  # the producer
        got = [o.clone() for o in run(bufs)]  # the call, then the consumer
    side.synchronize()
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a), _bits(b)), name
    torch.cuda.synchronize()


# ---- the meter -----------------------------------------------------------------------------------------------------------------------------------

def test_meter_on_device_tensors_agrees_with_the_host_path_within_the_measured_tolerance(tmp_path):
    """One batch of two chains of the dipeptide with driven torsions (views of a [chains, n, T, 3] block) against 600 reference frames.
    The device's fp32 dihedral, cosf and sinf differ from numpy's in the last places; the tolerance is `_swd_cases.TOLERANCE`: ten times
    what moving the host path's float32 descriptors by their rounding bound does to a distance, measured on the CPU."""
    from jamun_amd.callbacks import SlicedWassersteinMetricsCallback

    dev = _dev()
    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, dev)
    device_cb, device_smp = meter_run(SlicedWassersteinMetricsCallback, tmp_path / "device", mol, batches, dev, xyz=ref, device="device")
    host_cb, host_smp = meter_run(SlicedWassersteinMetricsCallback, tmp_path / "host", mol, batches, dev, xyz=ref, device="host")
    meter = device_cb.meters["m"]
    assert meter._dev and not host_cb.meters["m"]._dev
    assert torch.is_tensor(meter.ref_sorted) and meter.ref_sorted.is_cuda and tuple(meter.ref_sorted.shape) == (20, sc.REFERENCE_T)
    assert torch.is_tensor(meter.joined_sorted) and tuple(meter.joined_sorted.shape) == (20, 2 * sc.CHAIN_T)
    dd, hd = tmp_path / "device" / "m" / "sliced_wasserstein", tmp_path / "host" / "m" / "sliced_wasserstein"
    names = sorted(os.listdir(dd))
    assert names == sorted(os.listdir(hd)) == ["0.npz", "1.npz", "joined.npz", "projections.npz"]
    assert open(dd / "projections.npz", "rb").read() == open(hd / "projections.npz", "rb").read()
    worst = 0.0
    for name in names[:-1]:
        a, b = np.load(dd / name), np.load(hd / name)
        assert sorted(a.files) == sorted(b.files) and np.array_equal(a["num_samples"], b["num_samples"]), name
        assert np.array_equal(a["nonfinite"], b["nonfinite"]) and (a["nonfinite"] == 0).all() and np.isfinite(a["ws_distance"]).all(), name
        assert a["w2sq_per_projection"].shape == b["w2sq_per_projection"].shape == (a["num_samples"].shape[0], 20), name
        worst = max(worst, float(np.abs(a["ws_distance"] - b["ws_distance"]).max()))
    print(f"device against host path: worst difference of a ws_distance {worst:.3e} (tolerance {sc.TOLERANCE:.3e})")
    assert worst <= sc.TOLERANCE
    assert np.load(dd / "joined.npz")["num_samples"].tolist() == [100, 200, 400, 500]
    key = "m/ws_distance/pred_traj_joined"
    assert abs(device_smp.fabric.logged[-1][key] - host_smp.fabric.logged[-1][key]) <= sc.TOLERANCE
    # on the kernel's own descriptors the specification gives the device path's keys bit for bit and its W2^2 within the summation bound
    x = native.internal_coords(batches[0][0]["xhat_traj"].transpose(0, 1), _up(meter.index, dev), cossin=True).cpu().numpy()
    x_ref = native.internal_coords(ref.to(dev), _up(meter.index, dev), cossin=True).cpu().numpy()
    kx, kr = swd.project_host(x, meter.proj_rows), swd.project_host(x_ref, meter.proj_rows)
    want = swd.w2sq_sorted_host(swd.sort_segments_host(kx, [sc.CHAIN_T]), swd.sort_segments_host(kr, [sc.REFERENCE_T]))
    got = np.load(dd / "0.npz")["w2sq_per_projection"][-1]
    assert (np.abs(got - want) <= sc.w2sq_bound(sc.CHAIN_T, sc.REFERENCE_T) * want).all()
    assert np.array_equal(_bits(meter.ref_sorted), _bits(swd.sort_segments_host(kr, [sc.REFERENCE_T])))


def test_meter_with_device_set_refuses_cpu_tensors(tmp_path):
    from jamun_amd.callbacks import SlicedWassersteinMetricsCallback

    mol = dipeptide()
    ref, batches = sc.meter_fixture(mol, torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"SlicedWassersteinMetrics\(device='device'\) needs float32 sample tensors on a GPU"):
        meter_run(SlicedWassersteinMetricsCallback, tmp_path, mol, batches, _dev(), xyz=ref, device="device")
