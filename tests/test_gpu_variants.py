"""GPU parity beyond the default hyper-parameter point (``-m gpu``): other depths, the separable architecture at its shipped depth,
the noise level / cutoff / normalisation of the reference's other experiment files, a narrower hidden representation, and a
"trained-like" weight distribution — each against cached CPU-oracle outputs (``tests/golden/make_oracle_fixtures.py: VARIANTS``,
which cites the reference file of every point).  Tolerances as ``test_gpu_parity.py``: x-hat <= 1e-5 nm RMSD, per-layer features
<= 2e-5 of the layer maximum, edge structure exact.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _select_cases as sel

pytestmark = pytest.mark.gpu

RMSD_TOL_NM = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _mk():
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", os.path.join(GOLDEN, "make_oracle_fixtures.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def _golden(name):
    return {k: torch.tensor(v) for k, v in np.load(os.path.join(GOLDEN, name + ".npz")).items()}


def rmsd(a, b):
    return ((a.double().cpu() - b.double().cpu()) ** 2).sum(-1).mean().sqrt().item()


# (variant, molecules, what jamun_sampler_stats must report — the kernels the case is meant to exercise; the default-width ones in
# _select_cases.py, where tests/test_select_host.py asks the host selection the same)
CASES = [
    ("nl2", "ragged", sel.VARIANT_STATS["nl2", "ragged"]),
    ("sep_nl4", "ragged", dict()),
    ("idrome", "ragged", dict(dg_emu=1)),
    ("idrome", "dense70", dict(dg_emu=1)),
    ("r1000", "ragged", dict(dg_emu=1)),
    ("h64x16", "ragged", dict()),
    ("trained", "chain17x6", sel.VARIANT_STATS["trained", "chain17x6"]),
    ("trained", "ragged", sel.VARIANT_STATS["trained", "ragged"]),
    ("trained", "chig93x2", sel.VARIANT_STATS["trained", "chig93x2"]),  # the reference's chignolin shape (93 heavy atoms) on k_conv_ml / k_conv_mlx
    ("sep_trained", "ragged", dict()),
    # the default point on BASELINE configs[1] as the reference runs it: 48 DISTINCT dipeptides (real topology, 143 distinct embedding rows)
    ("default", "dipep48", sel.VARIANT_STATS["default", "dipep48"]),
]


@pytest.mark.parametrize("variant,kind,want", CASES, ids=[f"{v}-{k}" for v, k, _ in CASES])
def test_forward_matches_oracle_at_other_hyperparameters(variant, kind, want):
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden(f"oracle_forward_{variant}_{kind}" if variant != "default" else f"oracle_forward_{kind}")
    sigma = mk.VARIANTS[variant]["sigma"]
    ck = mk.variant_checkpoint(variant)
    model = Denoiser.from_checkpoint_dict(ck).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules(kind)).to(dev)
    smp = model.sampler_for(batch, sigma)
    y = ref["y"].to(dev)
    x = smp.xhat(y)
    st = smp.stats()
    for k, v in want.items():
        assert st[k] == v, (k, st)
    assert torch.equal(smp.debug_read(1).cpu().flatten().long(), ref["deg"])
    assert st["n_edges"] == int(ref["n_edges"])
    if variant == "idrome":  # everything inside the cutoff: molecules above 33 atoms sit at torch_cluster's 32-neighbour cap
        deg = ref["deg"]
        assert int(deg.max()) >= 32 and (deg >= 32).float().mean() > 0.3
    n_layers = ck["hyper_parameters"]["arch"]["n_layers"]
    assert f"x{n_layers + 1}" not in ref
    for l in range(n_layers + 1 if "x0" in ref else 0):  # (the big cases cache no per-layer features)
        xl, r = smp.debug_read(0, l).cpu(), ref[f"x{l}"]
        err = (xl - r).abs().max().item() / max(r.abs().max().item(), 1e-6)
        assert err < 2e-5, (l, err)
        if variant.endswith("trained"):
            # per CHANNEL: the features of this preset spread over 2^+-10 between channels, so an error measured against the
            # layer maximum would say nothing about the small channels (which the next layer multiplies by large weights)
            cmax = r.abs().amax(0)
            cerr = ((xl - r).abs().amax(0) / cmax.clamp_min(1e-30)).max().item()
            assert cerr < 1e-4, (l, cerr)
    g = smp.debug_read(2).cpu()
    assert (g - ref["g"]).abs().max().item() < 2e-5 * max(ref["g"].abs().max().item(), 1.0)
    assert rmsd(x, ref["xhat"]) <= RMSD_TOL_NM, rmsd(x, ref["xhat"])
    s = smp.score(y)
    assert rmsd(s, ref["score"]) <= RMSD_TOL_NM / sigma**2


def test_trained_like_weights_through_every_f16x3_kernel_against_the_fp32_kernels(monkeypatch):
    """Kernel against kernel on the trained-like preset: the f16x3 paths (k_conv_mf, k_conv_mfi, k_node_update_h, k_edge_h16) against
    the general fp32 kernels (k_conv, k_node_update, k_edge_h) on the same input, block by block — per channel."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden("oracle_forward_trained_chain17x6")
    model = Denoiser.from_checkpoint_dict(mk.variant_checkpoint("trained")).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules("chain17x6")).to(dev)
    fast = NativeSampler(model._native, 0.04, batch, dev)
    st = fast.stats()
    assert st["dg_mode"] == 4 and st["init_path"] == 3 and st["dg_emu"] == 1
    general = NativeSampler(model._native, 0.04, batch, dev, tuning={"no_dg": 1, "node_fp32": 1, "edge_h_fp32": 1})
    assert general.stats()["conv_path"] == 0
    y = ref["y"].to(dev)
    fast.build_edges(y)
    general.build_edges(y)
    a0, b0 = fast.conv_block(0).cpu(), general.conv_block(0).cpu()
    worst = ((a0 - b0).abs().amax(0) / b0.abs().amax(0).clamp_min(1e-30)).max().item()
    for l in range(1, 6):
        x_in = ref[f"x{l - 1}"].to(dev)
        a, b = fast.conv_block(l, x_in).cpu(), general.conv_block(l, x_in).cpu()
        worst = max(worst, ((a - b).abs().amax(0) / b.abs().amax(0).clamp_min(1e-30)).max().item())
    assert worst < 5e-5, worst


def test_walk_with_trained_like_weights_matches_oracle():
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden("oracle_walk_baoab_trained_ag4_12")
    model = Denoiser.from_checkpoint_dict(mk.variant_checkpoint("trained", mk.GAINS["stable"])).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules("ag4")).to(dev)
    smp = model.sampler_for(batch, 0.04)
    steps = 12
    noise = ref["noise"]
    y, v = ref["y0"].to(dev).clone(), noise[1].to(dev).clone()
    params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
    y_traj, score_traj, xhat_traj, xhat = smp.walk("baoab", y, v, params, noise[2 : steps + 1].to(dev).contiguous(), 0, True)
    worst = max(rmsd(xhat_traj[t], ref["xhat_traj"][t]) for t in range(steps))
    assert worst <= RMSD_TOL_NM, worst


def test_walk_at_the_reference_chignolin_shape_with_trained_like_weights_matches_oracle():
    """93 heavy atoms (what the reference feeds the model for chignolin: data/_mdtraj.py:60,218) x 2 walkers, trained-like weights, six BAOAB
    walk-jump frames on k_conv_ml / k_conv_mlx against the oracle: every frame within 1e-5 nm."""
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden("oracle_walk_baoab_trained_chig93_6")
    model = Denoiser.from_checkpoint_dict(mk.variant_checkpoint("trained", mk.GAINS["stable"])).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules("chig93x2")).to(dev)
    smp = model.sampler_for(batch, 0.04)
    st = smp.stats()
    assert (st["dg_mode"], st["init_path"], st["ml_window"]) == (5, 5, 96), st
    steps = 6
    noise = ref["noise"]
    y, v = ref["y0"].to(dev).clone(), noise[1].to(dev).clone()
    params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
    y_traj, score_traj, xhat_traj, xhat = smp.walk("baoab", y, v, params, noise[2 : steps + 1].to(dev).contiguous(), 0, True)
    worst = max(rmsd(xhat_traj[t], ref["xhat_traj"][t]) for t in range(steps))
    assert worst <= RMSD_TOL_NM, worst


@pytest.mark.parametrize("kind", ["chain17x6", "ragged", "chig93x2", "chig166x2"])
def test_opt_in_reduced_precision_conv_is_bounded_and_never_the_default(kind):
    """``jamun_tuning.f16x1`` / ``Sampler(precision="bf16-true")``: the hidden-layer conv (k_conv_mf, k_conv_ml) with ONE f16 MFMA per fp32
    product (operands rounded to 11 bits, fp32 accumulation) instead of the three of the f16x3 scheme.  The default stays f16x3 (dg_emu 1) and
    meets 1e-5 nm; the opt-in mode reports dg_emu 2 and must stay within 1e-3 nm RMSD of the oracle's x-hat (measured 2.5e-5 .. 7.6e-5 nm with the
    strongly non-linear test checkpoint: the level of the reference's own TF32 GPU path, float32_matmul_precision = high)
    and clearly above the fp32 path's error — i.e. it really is the reduced arithmetic that ran."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler
    from jamun_amd.sampling import Sampler

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden(f"oracle_forward_{kind}")
    from jamun_amd import synth

    model = Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(output_gain=0.5)).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules(kind)).to(dev)
    y = ref["y"].to(dev)
    full = NativeSampler(model._native, 0.04, batch, dev)
    fast = NativeSampler(model._native, 0.04, batch, dev, tuning={"f16x1": 1})
    assert full.stats()["dg_emu"] == 1 and fast.stats()["dg_emu"] == 2 and fast.stats()["dg_mode"] == full.stats()["dg_mode"]
    e_full, e_fast = rmsd(full.xhat(y), ref["xhat"]), rmsd(fast.xhat(y), ref["xhat"])
    print(f"f16x1 {kind}: x-hat RMSD vs oracle {e_fast:.2e} nm (f16x3: {e_full:.2e})")
    assert e_full <= RMSD_TOL_NM and 10 * e_full < e_fast <= 1e-3, (e_full, e_fast)
    assert torch.equal(fast.xhat(y), fast.xhat(y))
    # the Python switch: Sampler(precision=...) sets it on the model, the default does not; other names still raise
    assert Sampler().reduced_precision is False and Sampler(precision="bf16-true").reduced_precision is True
    with pytest.warns(UserWarning):  # the reference's autocast names are numerically fp32 for sampling (_sampler.py:62): fp32 here too, with a warning
        assert Sampler(precision="bf16-mixed").reduced_precision is False
    with pytest.raises(NotImplementedError):
        Sampler(precision="64-true")
    model.reduced_precision = True
    assert model.sampler_for(batch, 0.04).stats()["dg_emu"] == 2
    model.reduced_precision = False
    assert model.sampler_for(batch, 0.04).stats()["dg_emu"] == 1


@pytest.mark.parametrize("over,msg", [
    (dict(irreps_hidden="136x0e + 16x1e"), "SeparableConv: input irreps wider than 128x0e + 32x1e"),
    (dict(edge_attr_dim=32), "only edge_attr_dim = 64 is supported"),
])
def test_separable_conv_outside_its_envelope_is_refused_at_create_with_the_reason(over, msg):
    """``k_sep_fused`` / ``k_sep_linear`` cover the shipped ``e3conv_separable.yaml`` and its neighbourhood (<= 128 scalar /
    32 vector input channels, <= 64 edge slots, 64 radial hidden units); anything else fails in ``jamun_sampler_create`` with the reason in
    the message — there is no slower path to fall back to, and none is taken silently."""
    from jamun_amd import synth
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    mk = _mk()
    dev = torch.device("cuda", 0)
    batch = WalkerBatch.from_molecules(mk.molecules("ag4")).to(dev)
    import re

    with pytest.raises(RuntimeError, match=re.escape(msg)):
        model = Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(arch=synth.default_arch(**over), separable=True)).to(dev)
        model.sampler_for(batch, 0.04)


def test_reduced_precision_walks_stay_near_the_fp32_oracle_on_contractive_checkpoints():
    """The opt-in f16x1 conv over whole BAOAB walks (trained-like weights, contractive gain): 12 frames on the AG batch (k_conv_mf) and six on
    the 93-atom batch (k_conv_ml) against the fp32 oracle's trajectories — every frame within 1e-3 nm (measured 1e-5 .. 1e-4), none within the
    fp32 path's 1e-5 nm on every frame by accident of the test (the mode really ran)."""
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    mk = _mk()
    dev = torch.device("cuda", 0)
    model = Denoiser.from_checkpoint_dict(mk.variant_checkpoint("trained", mk.GAINS["stable"])).to(dev)
    for fixture, kind, steps in (("oracle_walk_baoab_trained_ag4_12", "ag4", 12), ("oracle_walk_baoab_trained_chig93_6", "chig93x2", 6)):
        ref = _golden(fixture)
        batch = WalkerBatch.from_molecules(mk.molecules(kind)).to(dev)
        smp = NativeSampler(model._native, 0.04, batch, dev, tuning={"f16x1": 1})
        assert smp.stats()["dg_emu"] == 2
        noise = ref["noise"]
        y, v = ref["y0"].to(dev).clone(), noise[1].to(dev).clone()
        params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
        _, _, xhat_traj, _ = smp.walk("baoab", y, v, params, noise[2 : steps + 1].to(dev).contiguous(), 0, True)
        errs = [rmsd(xhat_traj[t], ref["xhat_traj"][t]) for t in range(steps)]
        print(f"f16x1 walk {kind}: x-hat RMSD per frame {min(errs):.2e} .. {max(errs):.2e} nm")
        assert max(errs) <= 1e-3, errs
        assert max(errs) > 1e-7, errs


def test_long_chaotic_walk_agrees_with_the_oracle_as_an_ensemble():
    """The strongly non-linear checkpoint (gain 0.5: the bench checkpoint) amplifies any fp32 rounding difference ~4x per 5 steps, so beyond
    ~40 steps no fp32 implementation follows the oracle's single trajectories (tests/test_oracle.py::test_fp32_oracle_leaves_fp64_trajectory).
    What has to survive is the ENSEMBLE: 32 AG walkers x 80 BAOAB walk-jump frames on the same noise; the first frames are held to 1e-5 nm,
    and over frames 40..79 — where the trajectories have separated — the ensemble means of |x-hat - y| per atom, of the bonded distances of
    x-hat and of its radius of gyration must agree with the oracle's within five standard errors (walkers as independent samples)."""
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    mk = _mk()
    dev = torch.device("cuda", 0)
    ref = _golden("oracle_walk_baoab_ag32_80_strong")
    mols = mk.molecules("ag32")
    model = Denoiser.from_checkpoint_dict(mk.variant_checkpoint("default", mk.GAINS["strong"])).to(dev)
    batch = WalkerBatch.from_molecules(mols).to(dev)
    smp = model.sampler_for(batch, 0.04)
    steps = 80
    noise = ref["noise"]
    y, v = ref["y0"].to(dev).clone(), noise[1].to(dev).clone()
    params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
    y_traj, _, xhat_traj, _ = smp.walk("baoab", y, v, params, noise[2 : steps + 1].to(dev).contiguous(), 0, True)
    y_traj, xhat_traj = y_traj.cpu().double(), xhat_traj.cpu().double()
    errs = [rmsd(xhat_traj[t], ref["xhat_traj"][t]) for t in range(steps)]
    assert max(errs[:8]) <= RMSD_TOL_NM, errs[:8]
    n = mols[0]["pos"].shape[0]
    bonds = mols[0]["bonds"].long()

    W = len(mols)

    def stats(yt, xt):  # -> [3 observables][walkers]: means over frames 40.. and the walker's atoms / bonds
        yt, xt = yt[40:steps].reshape(-1, W, n, 3), xt[40:steps].reshape(-1, W, n, 3)
        disp = (xt - yt).norm(dim=-1).mean(dim=(0, 2))
        bl = (xt[:, :, bonds[0]] - xt[:, :, bonds[1]]).norm(dim=-1).mean(dim=(0, 2))
        rg = (xt - xt.mean(dim=2, keepdim=True)).pow(2).sum(-1).mean(dim=2).sqrt().mean(dim=0)
        return torch.stack([disp, bl, rg])

    a, b = stats(y_traj, xhat_traj), stats(ref["y_traj"].double(), ref["xhat_traj"].double())
    for name, ga, gb in zip(("|xhat - y|", "bond length of xhat", "radius of gyration of xhat"), a, b):
        # HIP and oracle walk on the SAME noise: walker w of one is paired with walker w of the other, so the standard error of the difference
        # of the means is that of the per-walker differences (treating the two ensembles as independent would overstate it)
        se = ((ga - gb).var(unbiased=True) / W).sqrt().item()
        d = abs((ga - gb).mean().item())
        print(f"ensemble {name}: HIP {ga.mean().item():.6f} oracle {gb.mean().item():.6f} nm, |diff| {d:.2e}, standard error {se:.2e}")
        assert d <= 5 * se + 1e-6, (name, d, se)
    print(f"single trajectories: x-hat RMSD vs oracle {errs[7]:.1e} nm at frame 7, {errs[39]:.1e} at 39, {errs[79]:.1e} at 79")


@pytest.mark.parametrize("kind", ["chain17x6", "chain33x4", "chig93x2"])
def test_create_time_self_check_passes_on_this_build_and_fires_on_a_corrupted_kernel(kind):
    """jamun_sampler_create runs the sampler's first forward (synthetic positions) through the kernels it selected AND through the general
    kernels and refuses to hand out a sampler whose node features differ by more than 2e-5 (jamun_api.cpp: sampler_self_check): a build whose
    matrix-formed kernels compute something else — the round-5 inline-asm hazard was such a build — must not sample.  Here: the default
    build passes (k_conv_mf + k_conv_mfi, + tail tiles, k_conv_ml + k_conv_mlx); with `selfcheck = 2` 4 KB of the selected conv kernel's
    weight stream are zeroed before the check, and create must fail with the reason; `selfcheck = -1` switches the check off."""
    from jamun_amd import synth
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    mk = _mk()
    dev = torch.device("cuda", 0)
    model = Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(output_gain=0.5)).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules(kind)).to(dev)
    ok = NativeSampler(model._native, 0.04, batch, dev)  # (default: check on)
    assert ok.stats()["conv_path"] == 2 and ok.stats()["dg_mode"] in (4, 5)
    with pytest.raises(RuntimeError, match="self-check failed.*must not sample"):
        NativeSampler(model._native, 0.04, batch, dev, tuning={"selfcheck": 2})
    off = NativeSampler(model._native, 0.04, batch, dev, tuning={"selfcheck": -1})
    ref = _golden(f"oracle_forward_{kind}")
    assert torch.equal(off.xhat(ref["y"].to(dev)), ok.xhat(ref["y"].to(dev)))  # the check leaves no trace in the sampler it passed
    with pytest.raises(RuntimeError, match="selfcheck"):
        NativeSampler(model._native, 0.04, batch, dev, tuning={"selfcheck": 7})


@pytest.mark.parametrize("kind", ["ag4", "chain17x6", "chain33x4", "ragged", "chig93x2", "chig166x2"])
def test_transposed_pre_pass_kernels_agree_bit_for_bit(kind):
    """k_tprod_t (round 6: a workgroup's four waves share a hidden unit's weight blocks through LDS, the rows are fetched whole and held as B
    fragments, T rows are stored as whole 128-byte lines) forms the same products in the same order as k_tprod_h's transposed branch
    (`jamun_tuning.no_tprod_t`), with powers of two for every scale: x-hat and score are bit-identical — also where the last workgroup's waves
    have fewer than 64 atoms or none (102, 132, .. atoms) and where the hidden units do not divide into the workgroups' runs."""
    from jamun_amd import synth
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    mk = _mk()
    dev = torch.device("cuda", 0)
    model = Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(output_gain=0.5)).to(dev)
    batch = WalkerBatch.from_molecules(mk.molecules(kind)).to(dev)
    new = NativeSampler(model._native, 0.04, batch, dev)
    old = NativeSampler(model._native, 0.04, batch, dev, tuning={"no_tprod_t": 1})
    if new.stats()["dg_mode"] not in (4, 5):
        pytest.skip("this shape does not take the transposed pre-pass")
    y = _golden(f"oracle_forward_{kind}")["y"].to(dev)
    assert torch.equal(new.xhat(y), old.xhat(y))
    assert torch.equal(new.score(y), old.score(y))
