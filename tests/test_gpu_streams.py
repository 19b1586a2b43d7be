"""GPU tests of the stream contract of ``include/jamun_hip.h``: all work of an entry point is queued on the stream passed in, with no
internal synchronisation unless stated.  Every entry point runs on a ``torch.cuda.Stream`` (which does not synchronise with the null
stream) behind busy work and a producer that overwrites its stale inputs in place, and in front of a consumer on the same stream; two
streams run at once; the entry points that say they synchronise are held to it.  The reference is the project's own serial behaviour (the
same call on the default stream, the device synchronised before and after) and every comparison is ``torch.equal``: one launch, memset,
copy or event record queued on the null stream instead reads its input early or writes its output late, and the bits differ.  The cases
are those of _stream_cases.py; test_stream_cases_host.py shows on the CPU that their stale inputs always change the result.

THE BUSY WORK.  `BUSY_STEPS` = 40 products of two `BUSY_N` x `BUSY_N` = 4096 x 4096 fp32 matrices in front of the producer.  Measured once on
an MI355X with stream events: the chain takes 36.6 ms.  No event can be put in front of a call's first kernel, so the time from enqueue to
first kernel start was bounded from above by the events around the whole first call of each group on an idle side stream: 304 us for the
sampler's forward (the slowest group; its host enqueue takes 80 to 110 us), 17 us for an operator, 30 us for an encoder.  The chain is 120
times the largest of them.  One control per group issues the call under test under the default stream and asserts that the result then
differs from the serial one; with a chain of 22 ms (24 products) the sampler's control did not see the misplaced call, with 36.6 ms all
three do.  The side streams are chosen so that the null stream demonstrably overtakes them (the `busy` fixture says why).
"""
import pytest
import torch

import _stream_cases as stc
from _frames_common import _dev

pytestmark = pytest.mark.gpu

BUSY_N, BUSY_STEPS = 4096, 40
BUSY_MS_MEASURED, START_US_MEASURED = 36.6, 304.0  # (the module docstring)


# ------------------------------------------------------------------------------------------------------------------------------ harness

class _SentinelTorch:
    """``torch`` as jamun_amd.native sees it during these tests: ``empty`` / ``empty_like`` hand out memory pre-filled ON THE CURRENT STREAM
    with a sentinel, so that an output the caching allocator recycles from the serial run cannot hold the right answer already."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    @staticmethod
    def _fill(t):
        if t.is_cuda and t.numel():
            t.fill_(12345.0 if t.is_floating_point() else 0x5A)
        return t

    def empty(self, *a, **k):
        return self._fill(self._real.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(self._real.empty_like(*a, **k))


@pytest.fixture(autouse=True)
def sentinel_outputs(monkeypatch):
    from jamun_amd import native

    monkeypatch.setattr(native, "torch", _SentinelTorch(torch))
    yield
    torch.cuda.synchronize()


class _Busy:
    def __init__(self, dev):
        g = torch.Generator().manual_seed(0)
        self.a = (torch.randn(BUSY_N, BUSY_N, generator=g) / BUSY_N ** 0.5).to(dev)
        self.out = [torch.empty_like(self.a) for _ in range(2)]  # (one per stream of the two-stream tests)

    def __call__(self, which=0, steps=BUSY_STEPS):
        for _ in range(steps):
            torch.mm(self.a, self.a, out=self.out[which])


def _overtaken_by_the_null_stream(side, busy) -> bool:
    """Whether work queued on the null stream runs while ``side`` is busy: a flag set behind busy work on ``side`` still reads 0 there."""
    flag = torch.zeros(1, device=busy.a.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy(0, BUSY_STEPS // 4)
        flag.fill_(1.0)
    seen = flag.clone()  # (on the null stream)
    torch.cuda.synchronize()
    return seen.item() == 0.0


@pytest.fixture(scope="module")
def busy():
    """The busy work, and with it the two side streams of this module (``busy.streams``).  HIP spreads its streams over a few hardware
    queues (four by default), and a side stream that shares the null stream's queue runs in submission order with it: there a launch on the
    wrong stream cannot be told from one on the right stream.  So streams are taken from torch's pool until two are found that the null
    stream overtakes; all tests of this module run on those two."""
    dev = _dev()
    b = _Busy(dev)
    b()  # (the first product loads the BLAS kernels: not inside a test's stream section)
    torch.cuda.synchronize()
    b.streams, tried = [], 0
    while len(b.streams) < 2 and tried < 16:
        side, tried = torch.cuda.Stream(dev), tried + 1
        if _overtaken_by_the_null_stream(side, b):
            b.streams.append(side)
    print(f"side streams: {len(b.streams)} of {tried} pool streams tried run independently of the null stream")
    assert len(b.streams) == 2, "no side stream runs independently of the null stream: these tests would see nothing"
    return b


@pytest.fixture(scope="module")
def samplers():
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    dev = _dev()
    cache = {}

    def build(name):
        _, _, tuning, _ = stc.SAMPLERS[name]
        model = Denoiser.from_checkpoint_dict(stc.sampler_checkpoint(name)).to(dev)
        batch = WalkerBatch.from_molecules(list(stc.sampler_molecules(name))).to(dev)
        return NativeSampler(model._native, stc.SIGMA, batch, dev, tuning=tuning)

    def get(name, twin=False, fresh=False):
        if fresh:
            return build(name)
        if (name, twin) not in cache:
            smp = cache[name, twin] = build(name)
            st = smp.stats()
            assert stc.SAMPLERS[name][3](st), (name, st)  # the path this sampler is there for
        return cache[name, twin]

    yield get
    cache.clear()


def _same(a, b) -> bool:
    """``torch.equal``; a NaN (a histogram prefix without a count) equals the NaN of the same bits."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if torch.equal(a, b):
        return True
    if not a.is_floating_point():
        return False
    bits = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _upload(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def _serial(case, true, fix):
    from jamun_amd import native

    torch.cuda.synchronize()
    bufs = {k: v.clone() for k, v in true.items()}
    torch.cuda.synchronize()
    want = [o.clone() for o in case.run(native, bufs, fix)]
    torch.cuda.synchronize()
    return want


def _on_side_stream(case, true, stale, fix, busy, misplaced=False):
    """Busy work, the producer, the call under test and the consumer, all on one side stream (the call under the default stream if
    ``misplaced``); only that stream is synchronised.  Returns the consumer's clones."""
    from jamun_amd import native

    dev = _dev()
    bufs = {k: v.clone() for k, v in stale.items()}
    torch.cuda.synchronize()
    side = busy.streams[0]
    with torch.cuda.stream(side):
        busy()
        for k in bufs:
            bufs[k].copy_(true[k])  # the producer: the true values, in place
        if misplaced:
            with torch.cuda.stream(torch.cuda.default_stream(dev)):
                outs = case.run(native, bufs, fix)
        else:
            outs = case.run(native, bufs, fix)
        got = [o.clone() for o in outs]  # the consumer
    side.synchronize()
    return got


def _check_ordered(case, fix, busy):
    dev = _dev()
    true, stale = _upload(case.inputs("true"), dev), _upload(case.inputs("stale"), dev)
    want = _serial(case, true, fix)
    got = _on_side_stream(case, true, stale, fix, busy)
    assert len(got) == len(want) >= 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), (case, i)


def _check_control(case, fix, busy):
    dev = _dev()
    true, stale = _upload(case.inputs("true"), dev), _upload(case.inputs("stale"), dev)
    want = _serial(case, true, fix)
    got = _on_side_stream(case, true, stale, fix, busy, misplaced=True)
    torch.cuda.synchronize()
    assert not all(_same(a, b) for a, b in zip(got, want)), f"{case}: a call on the wrong stream went unnoticed — the busy work is too short"


# ------------------------------------------------------------------------ 1. behind the producer, in front of the consumer

@pytest.mark.parametrize("sampler,op", stc.SAMPLER_CASES, ids=[f"{s}-{o}" for s, o in stc.SAMPLER_CASES])
def test_sampler_calls_on_a_side_stream_are_ordered_on_it(samplers, busy, sampler, op):
    _check_ordered(stc.sampler_case(sampler, op), {"smp": samplers(sampler)}, busy)


@pytest.mark.parametrize("case", stc.OPERATOR_CASES, ids=repr)
def test_operators_on_a_side_stream_are_ordered_on_it(busy, case):
    _check_ordered(case, _upload(case.fixed(), _dev()), busy)


@pytest.mark.parametrize("case", stc.ANALYSIS_CASES, ids=repr)
def test_encoders_and_analysis_on_a_side_stream_are_ordered_on_it(busy, case):
    _check_ordered(case, _upload(case.fixed(), _dev()), busy)


def test_control_a_sampler_call_on_the_wrong_stream_is_seen(samplers, busy):
    sampler, op = stc.CONTROLS["sampler"]
    _check_control(stc.sampler_case(sampler, op), {"smp": samplers(sampler)}, busy)


def test_control_an_operator_on_the_wrong_stream_is_seen(busy):
    case = stc.case_by_name(stc.OPERATOR_CASES, stc.CONTROLS["operators"])
    _check_control(case, _upload(case.fixed(), _dev()), busy)


def test_control_an_analysis_call_on_the_wrong_stream_is_seen(busy):
    case = stc.case_by_name(stc.ANALYSIS_CASES, stc.CONTROLS["analysis"])
    _check_control(case, _upload(case.fixed(), _dev()), busy)


# --------------------------------------------------------------------------------- 2. entry points that say they synchronise, do

def _walk_inputs(name, dev):
    return _upload(stc.sampler_case(name, "walk_baoab_noise").inputs("true"), dev)


def _queue_walk(smp, inp):
    return stc.SAMPLER_OPS["walk_baoab_noise"][1](None, inp, {"smp": smp})


def test_stats_check_and_profile_read_leave_the_side_stream_idle(samplers, busy):
    dev = _dev()
    smp = samplers("ag4")
    side = busy.streams[0]
    for call in (smp.stats, smp.check):
        inp = _walk_inputs("ag4", dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            busy()
            _queue_walk(smp, inp)
            assert not side.query()  # (the walk is still queued: the call below has something to wait for)
            call()
            assert side.query(), call.__name__
    profiles = []
    for stream in (side, torch.cuda.default_stream(dev)):
        inp = _walk_inputs("ag4", dev)
        torch.cuda.synchronize()
        smp.profile_enable(True)
        with torch.cuda.stream(stream):
            if stream is side:
                busy()
            _queue_walk(smp, inp)
            profiles.append(smp.profile_read())
            assert stream.query()
        smp.profile_enable(False)
    on_side, on_default = profiles
    assert {k: n for k, (_, n) in on_side.items()} == {k: n for k, (_, n) in on_default.items()}
    assert sum(n for _, n in on_side.values()) > 0
    for prof in profiles:
        for k, (ms, n) in prof.items():
            assert (ms > 0) == (n > 0), (k, ms, n)


# ------------------------------------------------------------------------------------------------------------- 3. two streams at once

def _serial_walk(smp, name, dev):
    inp = _walk_inputs(name, dev)
    torch.cuda.synchronize()
    want = [o.clone() for o in _queue_walk(smp, inp)]
    torch.cuda.synchronize()
    return want


@pytest.mark.parametrize("pair", [("ag4", "chig93x2"), ("ag4", "ag4")], ids=["different_paths", "same_model_and_topology"])
def test_two_samplers_walk_on_two_streams_at_once(samplers, busy, pair):
    dev = _dev()
    smps = [samplers(pair[0]), samplers(pair[1], twin=pair[0] == pair[1])]
    assert smps[0] is not smps[1]
    want = [_serial_walk(s, n, dev) for s, n in zip(smps, pair)]
    inps = [_walk_inputs(n, dev) for n in pair]
    streams = busy.streams
    torch.cuda.synchronize()
    got = []
    for i in (0, 1):  # both queued before either stream is synchronised
        with torch.cuda.stream(streams[i]):
            busy(i, BUSY_STEPS // 4)
            got.append([o.clone() for o in _queue_walk(smps[i], inps[i])])
    for s in streams:
        s.synchronize()
    for i in (0, 1):
        for j, (a, b) in enumerate(zip(got[i], want[i])):
            assert _same(a, b), (pair[i], j)


def _previous_trajectory(smp, dev):
    """24 x-hat frames of the first dipeptide of the ``ag4`` batch [24, 10, 3]: a view of the walk's frame-major trajectory."""
    from jamun_amd import native

    inp = _upload(stc.sampler_case("ag4", "walk_baoab_philox").inputs("true"), dev)
    params = native.make_mcmc_params(24, 0.04, 1.0, 1.0, 1.0, stc.WALK_CLIP)
    _, _, xhat_traj, _ = smp.walk("baoab", inp["y"], inp["v"], params, None, 7, True)
    torch.cuda.synchronize()
    assert xhat_traj.shape[0] == 24
    return xhat_traj[:, :10]


def _analysis_pipeline(native, frames, fix):
    """What the callbacks queue for a chain: both encoders, internal coordinates, the TICA and the MSM reductions."""
    out = stc._run_pdb(native, {"xyz": frames}, fix) + stc._run_dcd(native, {"xyz": frames}, fix)
    x = native.internal_coords(frames, fix["index"], cossin=True)
    sums, moments = native.lagged_moments(x, 2)
    proj = native.project_frames(x, fix["mean"], fix["v"])
    acf = native.autocov_sums(proj[:, 0], 5)
    labels, sqdist, _ = native.assign_centers(proj, fix["centers"], sqdist=True)
    counts, csums = native.cluster_sums(proj, labels, 4)
    trans = native.transition_counts(labels, 2, 4)
    occupancy = native.label_counts(labels, fix["bounds"], 4)
    return out + [x, sums, moments, proj, acf, labels, sqdist, counts, csums, trans, occupancy]


def test_a_sampler_walks_while_the_previous_trajectory_is_analysed_on_a_side_stream(samplers, busy):
    import numpy as np

    import _intcoord_cases as ic
    from jamun_amd import native
    from _traj_molecules import dipeptide

    dev = _dev()
    smp = samplers("ag4")
    frames = _previous_trajectory(smp, dev)
    index = ic.mixed_table(dipeptide()["pos"].numpy(), 5, seed=5)
    W = 2 * index.shape[0]
    fix = _upload(dict(stc._pdb_fixed(), index=torch.from_numpy(index), mean=stc._randn((W,), 1, torch.float64), v=stc._randn((W, 3), 2, torch.float64),
                       centers=stc._randn((4, 3), 3, torch.float64), bounds=torch.from_numpy(np.array([0, 10, 24], dtype=np.int32))), dev)
    torch.cuda.synchronize()
    want_analysis = [o.clone() for o in _analysis_pipeline(native, frames, fix)]
    torch.cuda.synchronize()
    want_walk = _serial_walk(smp, "ag4", dev)
    inp = _walk_inputs("ag4", dev)
    side = busy.streams[0]
    torch.cuda.synchronize()
    busy(0, BUSY_STEPS // 4)  # the current stream: the walk below is still queued while the side stream's calls are issued
    got_walk = [o.clone() for o in _queue_walk(smp, inp)]
    with torch.cuda.stream(side):
        busy(1, BUSY_STEPS // 4)
        got_analysis = [o.clone() for o in _analysis_pipeline(native, frames, fix)]
    side.synchronize()
    torch.cuda.current_stream(dev).synchronize()
    for j, (a, b) in enumerate(zip(got_analysis, want_analysis)):
        assert _same(a, b), ("analysis", j)
    for j, (a, b) in enumerate(zip(got_walk, want_walk)):
        assert _same(a, b), ("walk", j)


def test_lagged_moments_on_two_streams_keep_their_partial_sums_apart(busy):
    """`native._workspace`: one workspace per (device, stream).  Two calls on different inputs at once, then the same pair with more
    frames, so that both workspaces are replaced while the first pair may still be running."""
    from jamun_amd import native

    import _tica_cases as tc

    dev = _dev()
    small = [torch.from_numpy(tc.feature_rows(1100, 7, seed=s).copy()).to(dev) for s in (0, 1)]
    large = [torch.from_numpy(tc.feature_rows(9000, 7, seed=s).copy()).to(dev) for s in (2, 3)]
    torch.cuda.synchronize()
    want = []
    for x in small + large:
        want.append([o.clone() for o in native.lagged_moments(x, 5)])
        torch.cuda.synchronize()
    streams = busy.streams
    got = [None] * 4
    for i in (0, 1):
        with torch.cuda.stream(streams[i]):
            busy(i, BUSY_STEPS // 4)
            got[i] = [o.clone() for o in native.lagged_moments(small[i], 5)]
    sizes = [native._work[str(dev), int(s.cuda_stream)].numel() for s in streams]
    for i in (0, 1):
        with torch.cuda.stream(streams[i]):
            got[2 + i] = [o.clone() for o in native.lagged_moments(large[i], 5)]
    assert all(native._work[str(dev), int(s.cuda_stream)].numel() > n for s, n in zip(streams, sizes))  # (both grew)
    assert native._work[str(dev), int(streams[0].cuda_stream)].data_ptr() != native._work[str(dev), int(streams[1].cuda_stream)].data_ptr()
    for s in streams:
        s.synchronize()
    for i in range(4):
        for j, (a, b) in enumerate(zip(got[i], want[i])):
            assert _same(a, b), (i, j)


def test_one_sampler_forwards_on_two_streams_in_turn(samplers, busy):
    dev = _dev()
    smp = samplers("chig93x2")
    ys = [_upload(stc.sampler_case("chig93x2", "xhat").inputs(w), dev)["y"] for w in ("true", "stale")]
    torch.cuda.synchronize()
    want = []
    for y in ys:
        want.append(smp.xhat(y).clone())
        torch.cuda.synchronize()
    a, b = busy.streams
    with torch.cuda.stream(a):
        busy()
        first = smp.xhat(ys[0])
        done = torch.cuda.Event()
        done.record()
    with torch.cuda.stream(b):
        b.wait_event(done)
        second = smp.xhat(ys[1])
        second_copy = second.clone()
    b.synchronize()  # (b waited for a's event: a's forward is finished too)
    assert _same(second_copy, want[1])
    a.synchronize()
    assert _same(first, want[0])


# ------------------------------------------------------------------------------------------ 4. first use after create, on a side stream

def test_first_forward_after_create_on_a_fresh_side_stream_counts_what_the_default_stream_counts(samplers):
    dev = _dev()
    y = _upload(stc.sampler_case("chig93x2", "xhat").inputs("true"), dev)["y"]
    torch.cuda.synchronize()
    smp = samplers("chig93x2", fresh=True)  # (self-check on: the default)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        x_side = smp.xhat(y)
        st_side = smp.stats()
    torch.cuda.synchronize()
    other = samplers("chig93x2", fresh=True)
    x_default = other.xhat(y)
    st_default = other.stats()
    torch.cuda.synchronize()
    assert stc.SAMPLERS["chig93x2"][3](st_side)
    assert st_side == st_default
    assert st_side["conv_flop_exec_launch"] > 0
    assert _same(x_side, x_default)
