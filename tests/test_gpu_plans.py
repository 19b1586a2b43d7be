"""GPU tests (``-m gpu``): every work-list form the persistent conv kernels accept, against the general kernel and the oracle.

The parity suite runs the destination-grouped kernels on the default cut of their work lists only.  Here each kernel family runs under
every plan the host can emit — hidden-unit slices over XCD groups (jamun_tuning.dg_kgroups: segments carrying the left-over unit k_extra,
more than three partial slabs per atom for the node update) and other segment costs (seg_cost_tenths) — and the lists the kernels read are
copied back and checked with tests/test_plan.py's ``check_plan``."""
import numpy as np
import pytest
import torch

from jamun_amd import native
from test_gpu_parity import RMSD_TOL_NM, _ckpt, _golden, _mols, _oracle_setup, dev, rmsd  # noqa: F401  (dev: fixture)
from test_plan import check_plan

pytestmark = pytest.mark.gpu

# (jamun_tuning fields, on top of the kernel variant's); the first is the default plan
PLANS = [{}, {"dg_kgroups": 2}, {"dg_kgroups": 4}, {"dg_kgroups": 8}, {"seg_cost_tenths": -1}, {"seg_cost_tenths": 1}, {"seg_cost_tenths": 1000}]
# matrix-core forming (k_conv_mf / k_conv_ml, k_conv_mfi / k_conv_mfx / k_conv_mlx) and vector-ALU forming (k_conv_dg modes 0-3, k_conv_init_v)
VARIANTS = {"mfma": {}, "valu": {"no_mf": 1, "no_ml": 1, "no_mfi": 1}}
EXPECT = {  # (dg_mode, init_path) of the matrix-core variant
    "chain17x6": (4, 3), "chain33x4": (4, 3), "ragged": (4, 4), "dense70": (5, 5), "chig93x2": (5, 5), "chig166x2": (5, 5)}


def _weights(spans, dg_mode):
    """The sampler's tile weights (jamun_plan.cpp, select_kernels: 476 + 2 per 16 source rows, 24 in dg_mode 1)."""
    return 476 + (24 if dg_mode == 1 else 2) * ((spans[:, 1] - spans[:, 0] + 15) // 16)


def check_live_plan(smp):
    """check_plan on the lists the sampler's kernels read; also: the host planner export, run on the read-back tiles, plans the same
    lists.  Returns the forms seen (test_plan.FORMS)."""
    st = smp.stats()
    tab, meta = smp.debug_segments(3)
    tiles, spans = tab[:, :2], tab[:, 2:]
    _, chunk = np.unique(tiles[:, 0], return_inverse=True)  # (a destination chunk = the tiles of one destination range: source row blocks)
    tails, _ = smp.debug_segments(2)
    skip = np.isin(tiles[:, 0], tails[:, 1]) if len(tails) else np.zeros(len(tiles), bool)
    assert int(skip.sum()) == st["n_tail_tiles"]
    w = _weights(spans, st["dg_mode"])
    sc = meta["seg_cost_tenths"] / 10
    forms = set()
    for which, nsl in ((0, 4), (1, 5)):
        segs, m = smp.debug_segments(which)
        if m["n_values"] == 0:
            assert which == 1  # (the initial projector runs list 0)
            continue
        sk = skip if which == 0 else None
        atom_nslab, _ = smp.debug_segments(nsl)
        forms |= check_plan(segs, cus=m["grid"], ng=m["ng"], n_k=m["n_k"], n_atoms=smp.n_atoms, tiles=tiles, chunk=chunk, max_segs=m["max_segs"],
                            n_slabs=m["n_slabs"], atom_nslab=atom_nslab, skip=sk, weights=w, seg_cost=sc,
                            skipped_nslab=m["tail_runs"] if (which == 0 and skip.any()) else None, spans=spans)
        P = native.plan_segments(m["grid"], m["ng"], m["n_k"], smp.n_atoms, tiles, chunk, w, sk, sc)
        bare = segs.copy()
        bare[:, :, 1, 1:] = 0  # (the sampler embeds the tile descriptor into the second record)
        assert np.array_equal(P["segs"], bare), "the sampler's list differs from the host planner's on the same tiles"
        if which == 0:
            assert m["n_slabs"] == st["n_slices"]
    return forms


@pytest.fixture(scope="module")
def model(dev):
    from jamun_amd.model import Denoiser

    return Denoiser.from_checkpoint_dict(_ckpt("strong")).to(dev)


def _feats(smp):
    return [smp.debug_read(0, l).cpu() for l in range(6)]


def _feat_err(a, b):
    return max((x - y).abs().max().item() / max(y.abs().max().item(), 1e-6) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", list(EXPECT))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_plan_form_matches_the_general_kernel_and_the_oracle(dev, golden_dir, model, kind, variant):
    """Each (shape, kernel variant) under every plan: same kernels as the default plan, a valid plan read back, x-hat within 1e-5 nm of the
    cached oracle, node features after every block within 2e-5 x max of the general kernel and of the default plan, bit-reproducible."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.native import NativeSampler

    ref = _golden(golden_dir, f"oracle_forward_{kind}")
    batch = WalkerBatch.from_molecules(_mols(kind)).to(dev)
    y = ref["y"].to(dev)
    general = NativeSampler(model._native, 0.04, batch, dev, tuning={"no_dg": 1})
    xg, fg = general.xhat(y), _feats(general)
    base = VARIANTS[variant]
    paths, x0, f0 = None, None, None
    worst_g = worst_o = 0.0
    for plan in PLANS:
        smp = NativeSampler(model._native, 0.04, batch, dev, tuning={**base, **plan})
        st = smp.stats()
        p = (st["conv_path"], st["dg_mode"], st["init_path"])
        if paths is None:
            paths = p
            assert p[0] == 2
            if variant == "mfma":
                assert p[1:] == EXPECT[kind], p
            else:
                assert p[1] in (0, 1, 2, 3) and p[2] == 2, p
        assert p == paths, (plan, p, paths)  # (the switch changes the plan, not the kernels)
        forms = check_live_plan(smp)
        if plan.get("dg_kgroups", 1) > 1:
            assert "k_extra" in forms, plan
        if plan.get("dg_kgroups") == 8:
            assert st["n_slices"] > 3, st["n_slices"]  # (the node update's slab loop beyond the first three)
            print(f"PLANSTAT {kind} {variant} dg_kgroups=8 n_slices={st['n_slices']}")
        x = smp.xhat(y)
        f = _feats(smp)
        smp.check()
        assert torch.equal(smp.xhat(y), x), plan  # (bit-reproducible)
        assert rmsd(x, ref["xhat"]) <= RMSD_TOL_NM, (plan, rmsd(x, ref["xhat"]))
        assert rmsd(x, xg) <= RMSD_TOL_NM, plan
        eg = _feat_err(f, fg)
        assert eg <= 2e-5, (plan, eg)
        worst_g, worst_o = max(worst_g, eg), max(worst_o, rmsd(x, ref["xhat"]))
        if x0 is None:
            x0, f0 = x, f
        else:
            assert rmsd(x, x0) <= RMSD_TOL_NM, plan
            assert _feat_err(f, f0) <= 2e-5, plan
    print(f"PLANSTAT {kind} {variant} dg_mode={paths[1]} init_path={paths[2]} max_feat_err_vs_general={worst_g:.3e} "
          f"max_xhat_rmsd_vs_oracle={worst_o:.3e}")


def test_tail_tiles_under_sliced_plans(dev, model):
    """chain33x4 (dg_mode 4): 33-atom molecules cut into 32 + 1, the 1-atom tiles leave the hidden layers' lists (skipped tiles on the plan)
    for the tail kernels; with k-slices the partial-slab counts of tail and list atoms differ within one node-update workgroup."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.native import NativeSampler

    batch = WalkerBatch.from_molecules(_mols("chain33x4")).to(dev)
    for kg in (0, 2, 8):
        smp = NativeSampler(model._native, 0.04, batch, dev, tuning={"dg_kgroups": kg})
        st = smp.stats()
        assert st["dg_mode"] == 4 and st["n_tail_tiles"] > 0, st
        _, m1 = smp.debug_segments(1)
        print(f"PLANSTAT chain33x4 dg_kgroups={kg} n_tail_tiles={st['n_tail_tiles']} init_tail={m1['n_values'] == 0}")
        check_live_plan(smp)


# Plans with a segment that holds only the left-over hidden unit (k_run = 0, walk() cutting at i0 == base): found once on an MI355X (256 CUs)
# by creating samplers over segment costs; each case asserts that it keeps that form.
KRUN0_CASES = [("chain17x6", {"dg_kgroups": 2, "seg_cost_tenths": 5}), ("chig166x2", {"dg_kgroups": 4, "seg_cost_tenths": 2})]


@pytest.mark.parametrize("kind,tuning", KRUN0_CASES)
def test_segment_with_only_the_extra_unit(dev, golden_dir, model, kind, tuning):
    """k_conv_mf (chain17x6) and k_conv_ml (chig166x2) on a plan with a k_run = 0 segment: against the oracle and the general kernel."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.native import NativeSampler

    ref = _golden(golden_dir, f"oracle_forward_{kind}")
    batch = WalkerBatch.from_molecules(_mols(kind)).to(dev)
    y = ref["y"].to(dev)
    smp = NativeSampler(model._native, 0.04, batch, dev, tuning=tuning)
    forms = check_live_plan(smp)
    assert "k_run0" in forms, forms
    general = NativeSampler(model._native, 0.04, batch, dev, tuning={"no_dg": 1})
    x, xg = smp.xhat(y), general.xhat(y)
    smp.check()
    assert rmsd(x, ref["xhat"]) <= RMSD_TOL_NM and rmsd(x, xg) <= RMSD_TOL_NM
    err = _feat_err(_feats(smp), _feats(general))
    assert err <= 2e-5, err


@pytest.mark.parametrize("family", ["mf", "ml"])
def test_sliced_and_costless_plans_match_the_fp64_oracle(dev, family):
    """One random ragged batch per matrix-core family (dg_mode 4: molecules up to 57 atoms; dg_mode 5: 63..100 atoms) under dg_kgroups = 4
    and seg_cost_tenths = -1, against the oracle run live in float64."""
    import random

    from jamun_amd import synth
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler
    from oracle import denoiser as od

    rng = random.Random({"mf": 41, "ml": 42}[family])
    sizes = [rng.randint(2, 57) for _ in range(9)] if family == "mf" else [rng.randint(63, 100) for _ in range(3)] + [rng.randint(5, 40)]
    mols = [synth.random_chain(n, seed=500 + i) for i, n in enumerate(sizes)]
    ck = _ckpt("strong")
    topo, p, hp = _oracle_setup(mols, ck, dtype=torch.float64)
    torch.manual_seed(3)
    y = topo["pos"].double() + 0.04 * torch.randn(topo["pos"].shape, dtype=torch.float64)
    x_ref = od.xhat(y, topo, 0.04, p, hp)
    model = Denoiser.from_checkpoint_dict(ck).to(dev)
    batch = WalkerBatch.from_molecules(mols).to(dev)
    for plan in ({"dg_kgroups": 4}, {"seg_cost_tenths": -1}):
        smp = NativeSampler(model._native, 0.04, batch, dev, tuning=plan)
        assert smp.stats()["dg_mode"] == {"mf": 4, "ml": 5}[family]
        forms = check_live_plan(smp)
        if "dg_kgroups" in plan:
            assert "k_extra" in forms
        x = smp.xhat(y.float().to(dev))
        smp.check()
        r = rmsd(x, x_ref)
        print(f"PLANSTAT fp64 {family} {plan} xhat_rmsd={r:.3e}")
        assert r <= RMSD_TOL_NM, (plan, r)


@pytest.mark.parametrize("case,kind", [("oracle_walk_baoab_ag4_50", "ag4"), ("oracle_walk_baoab_chig93_6", "chig93x2")])
def test_fused_walk_with_sliced_lists_matches_oracle(dev, golden_dir, case, kind):
    """The persistent kernels re-read their lists on every launch: a whole fused walk under dg_kgroups = 4, every saved frame against the
    oracle as test_fused_walk_matches_oracle."""
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser
    from jamun_amd.native import NativeSampler

    ref = _golden(golden_dir, case)
    sigma = 0.04
    noise = ref["noise"]
    steps = noise.shape[0] - 1
    model = Denoiser.from_checkpoint_dict(_ckpt("stable")).to(dev)
    ns = NativeSampler(model._native, sigma, WalkerBatch.from_molecules(_mols(kind)).to(dev), dev, tuning={"dg_kgroups": 4})
    assert "k_extra" in check_live_plan(ns)
    params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
    y, v = ref["y0"].to(dev).clone(), noise[1].to(dev).clone()
    y_traj, score_traj, xhat_traj, xhat = ns.walk("baoab", y, v, params, noise[2 : 2 + steps - 1].to(dev).contiguous(), 0, True)
    ns.check()
    T = ref["y_traj"].shape[0]
    assert y_traj.shape[0] == T and xhat_traj.shape[0] == T and score_traj.shape[0] == ref["score_traj"].shape[0]
    worst = max(rmsd(xhat_traj[t], ref["xhat_traj"][t]) for t in range(T))
    assert worst <= RMSD_TOL_NM, worst
    assert rmsd(xhat, ref["xhat"]) <= RMSD_TOL_NM
    assert rmsd(y, ref["y"]) <= RMSD_TOL_NM
    assert max(rmsd(y_traj[t], ref["y_traj"][t]) for t in range(T)) <= RMSD_TOL_NM
    assert rmsd(v, ref["v"]) <= 1e-3
    assert rmsd(score_traj[-1], ref["score_traj"][-1]) <= RMSD_TOL_NM / sigma**2
