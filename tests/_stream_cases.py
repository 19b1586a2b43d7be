"""Case tables and input builders shared by ``test_stream_cases_host.py`` (CPU) and ``test_gpu_streams.py`` (GPU): every entry point of
``include/jamun_hip.h`` that takes a stream, as one `Case` each.

A `Case` names the buffers a producer overwrites in place (``inputs(which)``: ``"true"`` values and ``"stale"`` ones of the same shape and
type; stale values are finite and in range, so that a call that reads them too early gives a wrong answer and never a fault), the tables
that stay as they are (``fixed``: uploaded before anything is queued, because an upload from host memory waits for the stream and would
hide a launch on the wrong one), the call under test on device tensors (``run``) and the same operation under the host paths and the
oracle (``host``).  The host file asserts that stale and true inputs give different results under ``host``: a stale read is always visible.

The samplers of the sampler group are the smallest batches that select each conv path; `SAMPLERS` holds what ``jamun_sampler_stats`` must
report for each, and the host file asks ``jamun_debug_select_kernels`` the same.
"""
import functools
import os
import tempfile

import numpy as np
import torch

import _intcoord_cases as ic
import _msm_cases as mc
import _rama_cases as rc
import _select_cases as sel
import _sepconv_cases as sp
import _switch_cases as sc
import _tica_cases as tc
import _validity_cases as vc
from _traj_molecules import dipeptide, fill_template
from jamun_amd import synth

SIGMA = sc.SIGMA
WALK_STEPS, WALK_SAVE_EVERY, WALK_BURN_IN = 6, 2, 1
WALK_CLIP = sc.CLIP_BINDS  # binds: the scores of the test checkpoints are far longer than 3 per atom
WALK_SEED = 1234


class Case:
    def __init__(self, name, inputs, run, host, fixed=None):
        self.name, self.inputs, self.run, self.host = name, inputs, run, host
        self.fixed = fixed or (lambda: {})

    def __repr__(self):
        return self.name


def _t(a) -> torch.Tensor:
    return a.clone().contiguous() if torch.is_tensor(a) else torch.from_numpy(np.array(a, order="C"))


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _randn(shape, seed, dtype=torch.float32, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)).to(dtype)


# ---- samplers ------------------------------------------------------------------------------------------------------------------------------

def _tail_molecules():
    """``tails_1_to_8`` of test_tail_tiles_of_the_matrix_formed_conv cut to four molecules: tail tiles of 1, 2, 4 and 8 destinations."""
    return [synth.random_chain(n, seed=50 + i) for i, n in enumerate([33, 34, 36, 40])]


# name -> (architecture of _select_cases.ARCH_OVER, molecules, jamun_tuning, what jamun_sampler_stats must report)
SAMPLERS = {
    "ag4": ("conv", "ag4", None, lambda st: st["conv_path"] == 2 and st["dg_mode"] == 4 and st["init_path"] == 3),
    "tails": ("conv", "tails", None, lambda st: st["conv_path"] == 2 and st["dg_mode"] == 4 and st["n_tail_tiles"] >= 4 and st["n_tail"] == 15),
    "chig93x2": ("conv", "chig93x2", None, lambda st: st["conv_path"] == 2 and st["dg_mode"] == 5 and st["init_path"] == 5),
    "ragged_no_mf": ("conv", "ragged", {"no_mf": 1}, lambda st: st["conv_path"] == 2 and st["dg_mode"] in (0, 1, 2, 3) and st["init_path"] == 2),
    "ragged_no_dg": ("conv", "ragged", {"no_dg": 1}, lambda st: st["conv_path"] == 0 and st["dg_mode"] == -1 and st["init_path"] == 0),
    "separable": ("separable", "ag4", None, sp.is_separable),
    "wide": ("wide160", "ag4", None, sel.is_wide),
}


@functools.lru_cache(maxsize=None)
def sampler_molecules(name):
    kind = SAMPLERS[name][1]
    return tuple(_tail_molecules() if kind == "tails" else sel.molecules(kind))


@functools.lru_cache(maxsize=None)
def sampler_checkpoint(name):
    arch = SAMPLERS[name][0]
    if arch == "separable":
        return sp.checkpoint()
    return sc.checkpoint(arch_over=sel.ARCH_OVER[arch])


def feature_width(name) -> int:
    from jamun_amd.native import parse_hidden_irreps

    m0, m1 = parse_hidden_irreps(sampler_checkpoint(name)["hyper_parameters"]["arch"]["irreps_hidden"])
    return m0 + 3 * m1


def walk_params():
    from jamun_amd import native

    return native.make_mcmc_params(WALK_STEPS, 0.04, 1.0, 1.0, 1.0, WALK_CLIP, save_every_n_steps=WALK_SAVE_EVERY, burn_in_steps=WALK_BURN_IN)


@functools.lru_cache(maxsize=None)
def _sampler_arrays(name, which):
    topo = sc.collate(list(sampler_molecules(name)))
    n = topo["pos"].shape[0]
    if which == "true":
        y = sc.noisy_positions(topo, SIGMA, seed=11)
        seeds = (21, 22, 23)
    else:  # another draw, scaled by 1.5: other neighbourhoods, same shape
        y = 1.5 * sc.noisy_positions(topo, SIGMA, seed=12)
        seeds = (31, 32, 33)
    return dict(y=y.float().contiguous(), v=_randn((n, 3), seeds[0]), noise=_randn((WALK_STEPS - 1, n, 3), seeds[1]),
                x_in=_randn((n, feature_width(name)), seeds[2]))


def _sampler_inputs(name, keys):
    return lambda which: {k: _sampler_arrays(name, which)[k].clone() for k in keys}


def _walk(integrator, with_noise):
    def run(native, inp, fix):
        out = fix["smp"].walk(integrator, inp["y"], inp["v"], walk_params(), inp["noise"] if with_noise else None, WALK_SEED, True)
        assert all(o is not None for o in out)
        return [inp["y"], inp["v"], *out]

    return run


def _conv_blocks(native, inp, fix):
    smp = fix["smp"]
    smp.build_edges(inp["y"])
    return [smp.conv_block(0), smp.conv_block(1, inp["x_in"])]


@functools.lru_cache(maxsize=None)
def _oracle_xhat(name, which):
    from oracle import denoiser as od

    topo, p, hp = sc.oracle_setup(list(sampler_molecules(name)), sampler_checkpoint(name), torch.float32)
    return od.xhat(_sampler_arrays(name, which)["y"], topo, SIGMA, p, hp).numpy()


def _sampler_host(name, keys):
    """x-hat of the oracle on ``y``; what one B-A-O-A update makes of ``v`` and ``noise``; a scaled ``x_in`` (every block is linear in the
    features up to the gate, and the skip path alone carries them through)."""
    def host(inp):
        which = "true" if torch.equal(inp["y"], _sampler_arrays(name, "true")["y"]) else "stale"
        out = [_oracle_xhat(name, which)]
        k = sc.langevin_consts(0.04, 1.0, 1.0)
        if "v" in keys:
            zero = np.zeros_like(_np(inp["v"]))
            R = _np(inp["noise"])[0] if "noise" in keys else zero
            out += list(sc.np_baoab_pre(_np(inp["y"]), _np(inp["v"]), zero, R, k))
        if "x_in" in keys:
            out.append(_np(inp["x_in"]))
        return out

    return host


SAMPLER_OPS = {
    "xhat": (("y",), lambda native, inp, fix: [fix["smp"].xhat(inp["y"])]),
    "score": (("y",), lambda native, inp, fix: [fix["smp"].score(inp["y"])]),
    "walk_baoab_noise": (("y", "v", "noise"), _walk("baoab", True)),
    "walk_baoab_philox": (("y", "v"), _walk("baoab", False)),
    "walk_aboba_noise": (("y", "v", "noise"), _walk("aboba", True)),
    "conv_blocks_0_1": (("y", "x_in"), _conv_blocks),
}


def sampler_case(sampler, op) -> Case:
    keys, run = SAMPLER_OPS[op]
    return Case(f"{sampler}-{op}", _sampler_inputs(sampler, keys), run, _sampler_host(sampler, keys))


SAMPLER_CASES = [(s, op) for s in SAMPLERS for op in SAMPLER_OPS]


# ---- stand-alone operators (the sizes of their tests in test_gpu_parity.py / test_gpu_switches.py) ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _ragged():
    from jamun_amd.data import WalkerBatch

    return WalkerBatch.from_molecules(sel.molecules("ragged"))


def _positions(which):
    b = _ragged()
    return {"pos": (b.pos + 0.04 * _randn(tuple(b.pos.shape), 0)) * (1.0 if which == "true" else 1.5)}


def _ptr_fixed():
    return {"ptr": _ragged().ptr.to(torch.int32)}


def _host_mean_center(inp):
    from oracle import graph as og

    b = _ragged()
    return [og.mean_center(inp["pos"], b.batch, b.num_graphs).numpy()]


RADIUS = 0.58726


def _host_radius_graph(inp):
    from oracle import graph as og

    b = _ragged()
    return [torch.bincount(og.radius_graph(inp["pos"], RADIUS, b.batch)[1], minlength=b.num_nodes).numpy()]


@functools.lru_cache(maxsize=None)
def _segments(width=64, n_out=300):
    g = torch.Generator().manual_seed(1)
    counts = torch.randint(0, 40, (n_out,), generator=g)
    counts[7] = counts[n_out - 1] = 0
    seg = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    return seg.to(torch.int32), torch.repeat_interleave(torch.arange(n_out), counts), int(seg[-1]), n_out, width


def _host_scatter_mean(inp):
    from oracle import graph as og

    _, index, _, n_out, _ = _segments()
    return [og.scatter_mean(inp["src"], index, n_out).numpy()]


@functools.lru_cache(maxsize=None)
def _edges():
    mol = synth.random_chain(40, seed=4)
    g = torch.Generator().manual_seed(0)
    n = mol["pos"].shape[0]
    src, dst = torch.randint(0, n, (700,), generator=g), torch.randint(0, n, (700,), generator=g)
    src[5] = dst[5]
    return mol["pos"], torch.stack([src, dst])


def _host_edge_geometry(inp):
    from oracle import e3

    ei = _edges()[1]
    vec = inp["pos"][ei[0]] - inp["pos"][ei[1]]
    return [e3.spherical_harmonics_01(vec).numpy(), e3.soft_one_hot_linspace_gaussian(vec.norm(dim=1), 0.0, 0.587, 32).numpy()]


LINEAR = (120, 32, 152, 32)  # the head's Linear of test_node_linear_export_matches_oracle


def _host_node_linear(inp):
    from oracle import e3

    in0, in1, out0, out1 = LINEAR
    return [e3.linear(inp["x"], _randn((in0 * out0 + in1 * out1,), 2), [(in0, 0), (in1, 1)], [(out0, 0), (out1, 1)]).numpy()]


UPDATE_N = 257  # k_baoab_post4 and the remainder kernel
UPDATE = dict(delta=0.05, friction=0.7, M=2.0, beta=0.8, clip=3.0)


def update_params():
    from jamun_amd import native

    return native.make_mcmc_params(5, UPDATE["delta"], UPDATE["friction"], UPDATE["M"], UPDATE["beta"], UPDATE["clip"])


def _update_inputs(keys):
    def inputs(which):
        base = 100 if which == "true" else 200
        return {k: _randn((UPDATE_N, 3), base + i, scale=5.0 if k == "score" else 1.0) for i, k in enumerate(keys)}

    return inputs


def _run_baoab(native, inp, fix):
    p = update_params()
    native.baoab_pre(inp["y"], inp["v"], inp["psi"], inp["noise"], p)
    native.baoab_post(inp["v"], inp["psi"], inp["score"], p)
    return [inp["y"], inp["v"], inp["psi"]]


def _host_baoab(inp):
    a = {k: _np(v) for k, v in inp.items()}
    k = sc.langevin_consts(UPDATE["delta"], UPDATE["friction"], UPDATE["M"])
    y, v = sc.np_baoab_pre(a["y"], a["v"], a["psi"], a["noise"], k)
    v, psi = sc.np_baoab_post(v, a["score"], k, UPDATE["beta"], UPDATE["clip"])
    return [y, v, psi]


def _run_aboba(native, inp, fix):
    p = update_params()
    native.aboba_a(inp["y"], inp["v"], p)
    native.aboba_b(inp["y"], inp["v"], inp["score"], inp["noise"], p)
    return [inp["y"], inp["v"]]


def _host_aboba(inp):
    a = {k: _np(v) for k, v in inp.items()}
    k = sc.langevin_consts(UPDATE["delta"], UPDATE["friction"], UPDATE["M"])
    return list(sc.np_aboba_b(sc.np_aboba_a(a["y"], a["v"], k), a["v"], a["score"], a["noise"], k, UPDATE["beta"], UPDATE["clip"]))


PHILOX = (5000, 42, 3)  # atoms, seed, iteration

OPERATOR_CASES = [
    Case("mean_center", _positions, lambda native, inp, fix: [native.mean_center(inp["pos"], fix["ptr"])], _host_mean_center, _ptr_fixed),
    Case("radius_graph", _positions, lambda native, inp, fix: list(native.radius_graph(inp["pos"], RADIUS, fix["ptr"])), _host_radius_graph, _ptr_fixed),
    Case("scatter_mean", lambda which: {"src": _randn((_segments()[2], _segments()[4]), 3 if which == "true" else 4)},
         lambda native, inp, fix: [native.scatter_mean(inp["src"], fix["seg"], _segments()[3])], _host_scatter_mean, lambda: {"seg": _segments()[0]}),
    Case("edge_geometry", lambda which: {"pos": _edges()[0] * (1.7 if which == "true" else 2.5)},
         lambda native, inp, fix: list(native.edge_geometry(inp["pos"], fix["ei"], 0.587, 32)), _host_edge_geometry, lambda: {"ei": _edges()[1]}),
    Case("node_linear", lambda which: {"x": _randn((77, LINEAR[0] + 3 * LINEAR[1]), 5 if which == "true" else 6)},
         lambda native, inp, fix: [native.node_linear(inp["x"], fix["w"], *LINEAR)], _host_node_linear,
         lambda: {"w": _randn((LINEAR[0] * LINEAR[2] + LINEAR[1] * LINEAR[3],), 2)}),
    # (no input buffer: only the order in front of the consumer is at stake, and the host file has nothing stale to tell apart)
    Case("philox_normal", lambda which: {}, lambda native, inp, fix: [native.philox_normal(PHILOX[0], PHILOX[1], PHILOX[2], fix["anchor"].device)],
         lambda inp: [], lambda: {"anchor": torch.zeros(1)}),
    Case("baoab_pre_post", _update_inputs(("y", "v", "psi", "noise", "score")), _run_baoab, _host_baoab),
    Case("aboba_a_b", _update_inputs(("y", "v", "noise", "score")), _run_aboba, _host_aboba),
]


# ---- encoders and analysis (the smallest shapes of their case files that still take more than one workgroup) ------------------------------------

ENC_T = 7


def _frames10(which):
    return {"xyz": _randn((ENC_T, 10, 3), 1007 if which == "true" else 2007)}


@functools.lru_cache(maxsize=None)
def _pdb_template():
    from jamun_amd import pdb

    body, off = pdb.pdb_model_template(dipeptide())
    return body, off


def _pdb_fixed():
    body, off = _pdb_template()
    return {"body": torch.frombuffer(bytearray(body), dtype=torch.uint8).clone(), "off": torch.from_numpy(off.copy())}


def _run_pdb(native, inp, fix):
    dev = inp["xyz"].device
    need = native.pdb_models_nbytes(fix["body"].numel(), 0, inp["xyz"].shape[0])
    out = torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)  # (the caller zeroes the counter: on the stream of the call)
    assert native.encode_pdb_models(inp["xyz"], 0, fix["body"], fix["off"], out, cnt) == need
    return [out, cnt]


def _host_pdb(inp):
    body, off = _pdb_template()
    return [np.frombuffer(fill_template(body, off, inp["xyz"]), dtype=np.uint8)]


def _run_dcd(native, inp, fix):
    T, n = inp["xyz"].shape[0], inp["xyz"].shape[1]
    out = torch.full((T * 3 * (4 * n + 8),), 0xAB, dtype=torch.uint8, device=inp["xyz"].device)
    assert native.encode_dcd_frames(inp["xyz"], out) == out.numel()
    return [out]


def _host_dcd(inp):
    from jamun_amd import pdb

    with tempfile.TemporaryDirectory() as d:
        pdb.save_dcd(os.path.join(d, "a.dcd"), inp["xyz"])
        return [np.frombuffer(open(os.path.join(d, "a.dcd"), "rb").read()[276:], dtype=np.uint8)]


IC_T, IC_F = 65, 17  # one frame over a wave; one feature over a tile


@functools.lru_cache(maxsize=None)
def _rigid():
    frames, pos = ic.rigid_case()
    return np.array(frames[:IC_T], dtype=np.float32), ic.mixed_table(pos, IC_F, seed=IC_F)


def _rigid_inputs(which):
    frames, _ = _rigid()
    return {"frames": torch.from_numpy(frames.copy() if which == "true" else np.ascontiguousarray(frames[::-1] * np.float32(1.5)))}


def _rigid_fixed():
    frames, index = _rigid()
    return {"ref": torch.from_numpy(frames[0].copy()), "index": torch.from_numpy(index.copy())}


def _run_superpose_intcoord(native, inp, fix):
    aligned, rmsd = native.superpose_frames(inp["frames"], fix["ref"])
    return [aligned, rmsd, native.internal_coords(aligned, fix["index"], cossin=True)]  # (no host synchronisation in between)


def _host_superpose_intcoord(inp):
    from jamun_amd.features import internal_coords_host
    from jamun_amd.superpose import superpose_host

    frames, index = _rigid()
    aligned, rmsd = superpose_host(inp["frames"], frames[0])
    return [aligned, rmsd, internal_coords_host(aligned, index, cossin=True)]


HIST_T, HIST_W, HIST_BINS = 300, 4, 7
HIST_PAIRS = np.array([[0, 1], [2, 3], [1, 2]], dtype=np.int32)
HIST_CUTS = [63, 64, 65, 128, 299, 300]


def _hist_fixed():
    return {"pairs": torch.from_numpy(HIST_PAIRS.copy()), "ref": torch.from_numpy(rc.random_counts(1, 3, HIST_BINS, seed=9)[0].astype(np.int32))}


def _run_hist_js(native, inp, fix):
    counts, skipped = native.hist2d_pairs(inp["angles"], fix["pairs"], HIST_BINS, HIST_CUTS)
    return [counts, skipped, *native.js_divergence(counts, fix["ref"])]


def _host_hist_js(inp):
    from jamun_amd.ramachandran import histogram_host, js_divergence_host

    counts, _ = histogram_host(inp["angles"], HIST_PAIRS, HIST_BINS, HIST_CUTS)
    js = js_divergence_host(counts, rc.random_counts(1, 3, HIST_BINS, seed=9)[0])
    return [counts, js["pooled"], js["per_pair"]]


VAL_N, VAL_T = 33, 70  # one atom over the split between one and four waves per workgroup


@functools.lru_cache(maxsize=None)
def _validity_tables():
    from jamun_amd.validity import validity_tables

    return validity_tables(vc.helix(VAL_N), *vc.HELIX_TOLERANCES)


def _validity_fixed():
    from jamun_amd import native

    return {k: torch.from_numpy(a) for k, a in native.check_validity_tables(_validity_tables(), VAL_N).items()}


def _host_validity(inp):
    from jamun_amd.validity import validity_counts_host

    return list(validity_counts_host(inp["frames"], _validity_tables()))


TICA_T, TICA_W, TICA_LAG, TICA_D, ACF_LAG = 1100, 7, 5, 3, 40  # two slices of 1024 frames, the second partial


def _tica_inputs(which):
    return {"x": torch.from_numpy(tc.feature_rows(TICA_T, TICA_W, seed=0 if which == "true" else 1).copy())}


def _tica_fixed():
    return {"mean": _randn((TICA_W,), 7, torch.float64), "v": _randn((TICA_W, TICA_D), 8, torch.float64)}


def _host_moments(inp):
    from jamun_amd.tica import lagged_moments_host

    return list(lagged_moments_host(inp["x"], TICA_LAG))


def _host_project(inp):
    from jamun_amd.tica import project_host

    fix = _tica_fixed()
    return [project_host(inp["x"], fix["mean"].numpy(), fix["v"].numpy())]


def _host_autocov(inp):
    from jamun_amd.tica import autocov_sums_host

    return [autocov_sums_host(inp["y"], ACF_LAG)]


MSM_T, MSM_D, MSM_K, MSM_STATES, MSM_LAG = 1100, 3, 8, 6, 5
MSM_BOUNDS = np.array([0, 1, 400, 400, 1100], dtype=np.int32)


def _rows(which):
    return torch.from_numpy(mc.projection_rows(MSM_T, MSM_D, seed=0 if which == "true" else 1).copy())


def _labels(which):
    return torch.from_numpy(mc.labels_with_outliers(MSM_T, MSM_K, seed=0 if which == "true" else 1).copy())


def _centers_fixed():
    return {"centers": torch.from_numpy(mc.centers_for(mc.projection_rows(MSM_T, MSM_D), MSM_K))}


def _run_assign(native, inp, fix):
    labels, sqdist, _ = native.assign_centers(inp["y"], fix["centers"], sqdist=True)
    return [labels, sqdist]


def _host_assign(inp):
    from jamun_amd.msm import assign_centers_host

    return list(assign_centers_host(inp["y"], _centers_fixed()["centers"].numpy()))


def _host_cluster_sums(inp):
    from jamun_amd.msm import cluster_sums_host

    return list(cluster_sums_host(inp["y"], inp["labels"], MSM_K))


def _host_transitions(inp):
    from jamun_amd.msm import transition_counts_host

    return [transition_counts_host(inp["labels"], MSM_LAG, MSM_STATES)]


def _host_label_counts(inp):
    from jamun_amd.msm import label_counts_host

    return [label_counts_host(inp["labels"], MSM_BOUNDS, MSM_STATES)]


ANALYSIS_CASES = [
    Case("encode_pdb_models", _frames10, _run_pdb, _host_pdb, _pdb_fixed),
    Case("encode_dcd_frames", _frames10, _run_dcd, _host_dcd),
    Case("superpose_then_internal_coords", _rigid_inputs, _run_superpose_intcoord, _host_superpose_intcoord, _rigid_fixed),
    Case("hist2d_pairs_then_js_divergence",
         lambda which: {"angles": torch.from_numpy(rc.angle_table(HIST_T, HIST_W, HIST_BINS, seed=0 if which == "true" else 1).copy())},
         _run_hist_js, _host_hist_js, _hist_fixed),
    Case("validity_counts", lambda which: {"frames": torch.from_numpy(vc.noisy_frames(vc.helix(VAL_N)["pos"].numpy(), VAL_T, seed=1033 if which == "true" else 2033).copy())},
         lambda native, inp, fix: list(native.validity_counts(inp["frames"], fix)), _host_validity, _validity_fixed),
    Case("lagged_moments", _tica_inputs, lambda native, inp, fix: list(native.lagged_moments(inp["x"], TICA_LAG)), _host_moments),
    Case("project_frames", _tica_inputs, lambda native, inp, fix: [native.project_frames(inp["x"], fix["mean"], fix["v"])], _host_project, _tica_fixed),
    Case("autocov_sums", lambda which: {"y": _randn((TICA_T,), 40 if which == "true" else 41, torch.float64)},
         lambda native, inp, fix: [native.autocov_sums(inp["y"], ACF_LAG)], _host_autocov),
    Case("assign_centers", lambda which: {"y": _rows(which)}, _run_assign, _host_assign, _centers_fixed),
    Case("cluster_sums", lambda which: {"y": _rows(which), "labels": _labels(which)},
         lambda native, inp, fix: list(native.cluster_sums(inp["y"], inp["labels"], MSM_K)), _host_cluster_sums),
    Case("transition_counts", lambda which: {"labels": _labels(which)},
         lambda native, inp, fix: [native.transition_counts(inp["labels"], MSM_LAG, MSM_STATES)], _host_transitions),
    Case("label_counts", lambda which: {"labels": _labels(which)},
         lambda native, inp, fix: [native.label_counts(inp["labels"], fix["bounds"], MSM_STATES)], _host_label_counts,
         lambda: {"bounds": torch.from_numpy(MSM_BOUNDS.copy())}),
]

# the case of each group whose call the control issues on the wrong stream
CONTROLS = {"sampler": ("ag4", "xhat"), "operators": "mean_center", "analysis": "lagged_moments"}


def case_by_name(cases, name) -> Case:
    return next(c for c in cases if c.name == name)
