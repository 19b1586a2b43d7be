"""GPU tests (``-m gpu``) of the switches a checkpoint or a sampling config sets — the axis the other GPU files leave at its default.

1. Denoiser switches against the fp64 CPU oracle, run live (``tests/_switch_cases.py`` builds the checkpoints as a user's file would
   carry them; ``tests/test_switches_host.py`` asserts the CPU-side premise of every bound):
   * ``mean_center = False`` on translated walkers, through the default kernels, ``no_dg``, ``no_mf``, SeparableConv and the wide path,
     plus the closed form  xhat(y + t) - xhat(y) = c_skip t;
   * ``use_residue_sequence_index = True`` on both sides of the 32-row limit of the initial projectors, and the refusal of an index
     outside the embedding table;
   * ``w3j_111_sign = -1`` from negated ``_w3j_1_1_1`` buffers.  Pack sites and their consumers: ``build_layer`` (jamun_pack.cpp, the
     ``crosse`` entries: 1e x 1e -> 1e of the fully connected product) feeds every Conv kernel — k_conv (``no_dg``), k_conv_dg
     (``no_mf``), k_conv_mf, k_conv_ml, k_tail_form / k_tail_contract and k_conv_wide; ``build_layer_separable`` (``fac[4]``, the E
     columns) feeds k_sep_fused.  The initial projectors (2 k_conv_init_v, 3 k_conv_mfi, 4 k_conv_mfx, 5 k_conv_mlx, 0, 6) have scalar
     inputs only, so no signed weight reaches them: they run here in front of -1-packed hidden layers and must stay as they are;
   * the noise level: sigma 0.01 .. 1.0 (c_in, c_skip, c_out, the cutoff and c_noise all move).
2. The fused walks over a pairwise covering of their parameters, bit for bit against the stand-alone update kernels driven around the
   same native score, on guard-banded buffers.
3. The update kernels at their vector / remainder / unaligned seams against a NumPy float32 restatement.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _select_cases as sel
import _switch_cases as sc
from _switch_cases import RMSD_TOL_NM, SIGMA, rmsd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _model(ck):
    from jamun_amd.model import Denoiser

    return Denoiser.from_checkpoint_dict(ck).to(DEV)


def _sampler(model, mols, sigma=SIGMA, tuning=None):
    from jamun_amd.data import WalkerBatch
    from jamun_amd.native import NativeSampler

    return NativeSampler(model._native, sigma, WalkerBatch.from_molecules(mols).to(DEV), DEV, tuning=tuning)


def _oracle(mols, ck, y=None, sigma=SIGMA):
    from oracle import denoiser as od

    topo, p, hp = sc.oracle_setup(mols, ck, torch.float64)
    if y is None:
        y = sc.noisy_positions(topo, sigma)
    x, inter = od.xhat(y.double(), topo, sigma, p, hp, return_intermediates=True)
    return y, x, inter, hp


def _check_forward(smp, y, x_ref, inter, hp, sigma=SIGMA, bound=RMSD_TOL_NM):
    """The assertions of every switch: degrees and edge count exactly, per-block features within 2e-5 of the block maximum, x-hat within
    ``bound`` nm RMSD of the fp64 oracle and the score within ``bound / sigma^2``.  Returns the GPU's x-hat."""
    yd = y.to(DEV)
    x = smp.xhat(yd)
    deg = torch.bincount(inter["edge_index"][1], minlength=y.shape[0])
    assert torch.equal(smp.debug_read(1).cpu().flatten().long(), deg)
    assert smp.stats()["n_edges"] == inter["edge_index"].shape[1]
    for l in range(hp["n_layers"] + 1):
        xl, r = smp.debug_read(0, l).cpu().double(), inter[f"x{l}"]
        err = (xl - r).abs().max().item() / max(r.abs().max().item(), 1e-6)
        assert err < 2e-5, (l, err)
    e = rmsd(x, x_ref)
    print(f"x-hat RMSD against the fp64 oracle {e:.3e} nm (bound {bound:.1e})")
    assert e <= bound, e
    assert rmsd(smp.score(yd), (x_ref - y.double()) / sigma**2) <= bound / sigma**2
    return x


# (name, jamun_tuning, what jamun_sampler_stats must report) per architecture: _select_cases.py, which tests/test_select_host.py asks of the
# host selection as well
ARCH = {  # name -> (keyword arguments of sc.checkpoint, selections)
    "conv": (dict(), sel.CONV_SELECTIONS),
    "separable": (dict(separable=True), sel.SEPARABLE_SELECTIONS),
    "wide": (dict(arch_over=sel.WIDE_ARCH_H32), sel.WIDE_SELECTIONS),
}


# ---- 1. denoiser switches ------------------------------------------------------------------------------------------------------------


def _translated(topo, size=sc.TRANSLATION_NM):
    y = sc.noisy_positions(topo, SIGMA)
    return y, y + sc.walker_translations(topo["num_graphs"], size, topo["batch"])


def _assert_translation_law(smp, y, y_t):
    """xhat(y + t) - xhat(y) = c_skip t per walker without centring (g sees differences only), c_skip op for op in fp32 as
    jamun_sampler_create; compared on the fp32 inputs actually fed, within TRANSLATION_LAW_K * eps32 * max |y + t|
    (``_switch_cases.py`` derives the factor)."""
    dx = smp.xhat(y_t.to(DEV)).cpu().double() - smp.xhat(y.to(DEV)).cpu().double()
    law = float(sc.c_skip_fp32(SIGMA)) * (y_t.double() - y.double())
    bound = sc.TRANSLATION_LAW_K * sc.EPS32 * y_t.abs().max().item()
    err = (dx - law).abs().max().item()
    print(f"translation law: max deviation {err:.3e} nm (bound {bound:.3e})")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("arch", ["conv", "separable", "wide"])
@pytest.mark.parametrize("kind", ["chain17x6", "ragged", "chig93x2"])
def test_forward_without_centring_on_translated_walkers(kind, arch):
    """``mean_center: false`` in the checkpoint: geom_body / finalize_body skip the centroid, x-hat = c_skip y + c_out g follows the
    walker wherever it sits.  Every walker 8 nm from the origin in its own direction (the fp32 CPU oracle keeps a quarter of the
    tolerance there, test_switches_host.py), against the fp64 oracle under the same switch, through each kernel selection."""
    kw, selections = ARCH[arch]
    mols = sc.molecules(kind)
    ck_off, ck_on = sc.checkpoint(mean_center=False, **kw), sc.checkpoint(mean_center=True, **kw)
    topo = sc.oracle_setup(mols, ck_off)[0]
    y, y_t = _translated(topo)
    _, x_ref, inter, hp = _oracle(mols, ck_off, y_t)
    assert hp["mean_center"] is False
    model, centred = _model(ck_off), _model(ck_on)
    assert model._native.hparams_struct.mean_center == 0 and centred._native.hparams_struct.mean_center == 1
    for name, tuning, stats_ok in selections:
        smp = _sampler(model, mols, tuning=tuning)
        assert stats_ok(smp.stats()), (name, smp.stats())
        x = _check_forward(smp, y_t, x_ref, inter, hp)
        assert rmsd(x, _sampler(centred, mols, tuning=tuning).xhat(y_t.to(DEV))) >= sc.DID_SOMETHING, name  # the switch did something
        _assert_translation_law(smp, y, y_t)


def test_forward_without_centring_above_the_lds_budget_of_k_geom():
    """The global-memory path of geom_body / finalize_body (a 1100-atom walker beside two small ones) with ``mean_center = False``:
    finite, in-degrees equal to the stand-alone jamun_radius_graph on the UNcentred coordinates plus the bonds, and the translation law."""
    from jamun_amd import native

    mols = sc.molecules("big1100")
    topo = sc.collate(mols)
    y, y_t = _translated(topo)
    smp = _sampler(_model(sc.checkpoint(mean_center=False)), mols)
    x = smp.xhat(y_t.to(DEV))
    assert torch.isfinite(x).all()
    f = np.float32  # the sampler's cutoff on unscaled coordinates, fp32 op for op (jamun_sampler_create)
    s2 = f(SIGMA) * f(SIGMA)
    c_in = f(1.0) / np.sqrt(f(0.332) + f(6.0) * s2)
    r_cut = float(np.sqrt(f(1.0) + f(6.0) * s2) / c_in)
    ptr = topo["ptr"].to(torch.int32).to(DEV)
    _, deg_r = native.radius_graph(y_t.to(DEV), r_cut, ptr)
    bonded_in = torch.bincount(topo["bonds"][1], minlength=y.shape[0]).int()
    assert torch.equal(smp.debug_read(1).cpu().flatten().int(), deg_r.cpu() + bonded_in)
    _assert_translation_law(smp, y, y_t)


@pytest.mark.parametrize("kind", ["chain17x6", "ragged50", "chain17_shifted"])
def test_forward_with_the_residue_sequence_index(kind):
    """``use_residue_sequence_index: true``: the fourth embedding table is indexed by the atom's sequence index instead of row 0.  The
    distinct embedding rows — and with them the initial projector, k_conv_mfi (3) up to 32 rows, k_conv_mfx (4) above — are counted here
    from the (type, code, residue, sequence index) tuples: 16 rows either way, 105 either way, and 16 without / 48 with the switch."""
    mols = sc.molecules(kind)
    ck_on, ck_off = sc.checkpoint(use_residue_sequence_index=True), sc.checkpoint()
    y, x_ref, inter, hp = _oracle(mols, ck_on)
    assert hp["use_residue_sequence_index"] is True
    model, plain = _model(ck_on), _model(ck_off)
    assert model._native.hparams_struct.use_residue_sequence_index == 1
    for tuning, conv_path in ((None, 2), ({"no_dg": 1}, 0)):
        smp, off = _sampler(model, mols, tuning=tuning), _sampler(plain, mols, tuning=tuning)
        assert smp.stats()["conv_path"] == conv_path
        if tuning is None:
            assert smp.stats()["dg_mode"] == 4
            assert smp.stats()["init_path"] == sc.expected_init_path(mols, True), smp.stats()
            assert off.stats()["init_path"] == sc.expected_init_path(mols, False), off.stats()
        x = _check_forward(smp, y, x_ref, inter, hp)
        assert rmsd(x, off.xhat(y.to(DEV))) >= sc.DID_SOMETHING
    if kind == "chain17_shifted":
        assert (sc.expected_init_path(mols, False), sc.expected_init_path(mols, True)) == (3, 4)


def test_sequence_index_outside_the_table_is_refused():
    """A 57-atom chain numbers its residues up to 11 and the table has 10 rows: with the switch on creation fails with the reason;
    with it off (the index reads 0) the same batch samples."""
    mols = [sc.synth.random_chain(57, seed=4)]
    with pytest.raises(RuntimeError, match="index out of range for atom_embedder.residue_index_embedding.weight"):
        _sampler(_model(sc.checkpoint(use_residue_sequence_index=True)), mols)
    assert torch.isfinite(_sampler(_model(sc.checkpoint()), mols).xhat(mols[0]["pos"].to(DEV))).all()


SIGN_CASES = sel.FAMILY_CASES  # (molecules, architecture, [(name, tuning, stats predicate)])


@pytest.mark.parametrize("kind,arch,selections", SIGN_CASES, ids=[f"{k}-{a}" for k, a, _ in SIGN_CASES])
def test_forward_with_the_opposite_sign_of_w3j_111(kind, arch, selections):
    """A checkpoint whose e3nn buffers hold -epsilon / sqrt(6): the loader derives -1, both pack sites multiply the 1e x 1e -> 1e path
    by it, and every conv kernel that consumes such weights agrees with the fp64 oracle under the same sign — and differs from the same
    kernel under +1 by more than 100 tolerances."""
    kw = ARCH[arch][0]
    mols = sc.molecules(kind)
    ck_minus, ck_plus = sc.checkpoint(w3j_111_sign=-1.0, **kw), sc.checkpoint(**kw)
    y, x_ref, inter, hp = _oracle(mols, ck_minus)
    assert hp["w3j_111_sign"] == -1.0
    model, plus = _model(ck_minus), _model(ck_plus)
    assert model._native.hparams_struct.w3j_111_sign == -1.0 and plus._native.hparams_struct.w3j_111_sign == 1.0
    for name, tuning, stats_ok in selections:
        smp = _sampler(model, mols, tuning=tuning)
        assert stats_ok(smp.stats()), (name, smp.stats())
        x = _check_forward(smp, y, x_ref, inter, hp)
        assert rmsd(x, _sampler(plus, mols, tuning=tuning).xhat(y.to(DEV))) >= sc.DID_SOMETHING, name


@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("kind", ["ragged", "dense70"])
def test_forward_over_the_noise_levels(kind, sigma):
    """c_in, c_skip, c_out, the cutoff and c_noise are functions of sigma; the cutoff grows with it and ``dense70`` sits at the
    neighbour cap.  x-hat bound per level from the reference's own fp32 error (fp32 CPU oracle against fp64, measured in
    test_switches_host.py; the project's 1e-5 nm where that is at most 2.5e-6, four times it above — the kernels' f16x3 products carry
    about fp32 error in another summation order):

        sigma    ragged: oracle fp32 dev / bound     dense70: oracle fp32 dev / bound   (nm RMSD)
        0.01     3.5e-8 / 1e-5                       3.7e-8 / 1e-5
        0.1      1.5e-7 / 1e-5                       8.7e-8 / 1e-5
        0.4      4.2e-7 / 1e-5                       2.8e-7 / 1e-5
        1.0      3.9e-7 / 1e-5                       3.6e-7 / 1e-5
    """
    mols, ck = sc.molecules(kind), sc.checkpoint()
    y, x_ref, inter, hp = _oracle(mols, ck, sigma=sigma)
    smp = _sampler(_model(ck), mols, sigma=sigma)
    assert sel.default_kernels(smp.stats()), smp.stats()
    _check_forward(smp, y, x_ref, inter, hp, sigma=sigma, bound=sc.xhat_bound(kind, sigma))
    if kind == "dense70":
        assert int(torch.bincount(inter["edge_index"][1]).max()) >= 32


# ---- 2. the walk grid ----------------------------------------------------------------------------------------------------------------

SENTINEL = 7.25
_walk_samplers = {}


def _walk_sampler(batch, mean_center, no_fuse_geom):
    key = (batch, mean_center, no_fuse_geom)
    if key not in _walk_samplers:
        mols = sc.walk_molecules(batch)
        _walk_samplers[key] = (_sampler(_model(sc.checkpoint(gain=0.05, mean_center=mean_center)), mols, tuning={"no_fuse_geom": no_fuse_geom}), mols)
    return _walk_samplers[key]


class _Arena:
    """``frames`` frames of [n, 3] between two guard frames filled with a sentinel; ``ptr`` is None when the buffer is not passed."""

    def __init__(self, frames, n, passed=True):
        self.buf = torch.full((frames + 2, n, 3), SENTINEL, device=DEV)
        self.frames, self.passed = frames, passed
        self.ptr = int(self.buf[1].data_ptr()) if passed else None

    def body(self):
        return self.buf[1 : 1 + self.frames]

    def guards_untouched(self):
        g = torch.cat([self.buf[0], self.buf[1 + self.frames]])
        return bool((g == SENTINEL).all()) and (self.passed or bool((self.buf == SENTINEL).all()))


def _reference_walk(integrator, smp, y, v, params, noise, keep_y):
    """``sampling._python_walk`` with lists for results (it stacks them, which an empty trajectory does not survive): the stand-alone
    update kernels — pinned bit-exactly to the reference's baoab() / aboba() — around the sampler's own score."""
    from jamun_amd import native

    saves = lambda i: i % params.save_every_n_steps == 0 and i >= params.burn_in_steps  # noqa: E731
    y_traj = [y.clone()] if keep_y and saves(0) else []
    score_traj = []
    if integrator == "aboba":
        for i in range(1, params.steps):
            native.aboba_a(y, v, params)
            score = smp.score(y)
            native.aboba_b(y, v, score, noise[i - 1].contiguous(), params)
            if keep_y and saves(i):
                y_traj.append(y.clone())
                score_traj.append(score.clone())
        return y_traj, score_traj
    psi, score = torch.empty_like(y), smp.score(y)
    native.baoab_post(torch.zeros_like(v), psi, score, params)
    score_traj.append(score.clone())
    for i in range(1, params.steps):
        native.baoab_pre(y, v, psi, noise[i - 1].contiguous(), params)
        score = smp.score(y)
        native.baoab_post(v, psi, score, params)
        if keep_y and saves(i):
            y_traj.append(y.clone())
            score_traj.append(score.clone())
    return y_traj, score_traj


def _eq(a, frames):
    return a.shape[0] == len(frames) and all(torch.equal(a[t], f) for t, f in enumerate(frames))


@pytest.mark.parametrize("case", sc.WALK_CASES, ids=["-".join(str(v) for v in c) for c in sc.WALK_CASES])
def test_fused_walk_grid(case):
    import jamun_amd.sampling as S
    from jamun_amd import _lib, native

    integrator, steps, sb, clip_kind, noise_kind, traj, no_fuse, batch, mean_center, mcmc = case
    smp, mols = _walk_sampler(batch, mean_center, no_fuse)
    n = smp.n_atoms
    save_every, burn_in = sc.save_and_burn(sb, steps)
    M, friction, beta = sc.MCMC[mcmc]
    clip = {"none": None, "binds": sc.CLIP_BINDS, "loose": sc.CLIP_LOOSE}[clip_kind]
    params = native.make_mcmc_params(steps, 0.05, friction, M, beta, clip, save_every, burn_in)
    assert params.has_clip == int(clip is not None)
    g = torch.Generator().manual_seed(1000 + sc.WALK_CASES.index(case))
    topo = sc.collate(mols)
    y0 = topo["pos"] + SIGMA * torch.randn(n, 3, generator=g)
    if not mean_center:
        y0 = y0 + sc.walker_translations(topo["num_graphs"], 0.5, topo["batch"])  # (nothing centres these walkers)
    y0, v0 = y0.to(DEV), torch.randn(n, 3, generator=g).to(DEV)
    seed = 77 + steps
    if noise_kind == "tensor":
        noise = torch.randn(max(steps - 1, 0), n, 3, generator=g).to(DEV)
        ref_noise = noise
    else:  # the in-kernel Philox draws, reproduced by jamun_philox_normal
        noise = None
        ref_noise = torch.stack([native.philox_normal(n, seed, i, DEV) for i in range(1, steps)]) if steps > 1 else torch.zeros(0, n, 3, device=DEV)

    # frame counts: the reference's rule restated (sc.reference_frame_counts) AND jamun_num_frames, which is code under test
    ny, nsb, nsa = sc.reference_frame_counts(steps, save_every, burn_in)
    cy, cb, ca = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(smp._lib.jamun_num_frames(C.byref(params), C.byref(cy), C.byref(cb), C.byref(ca)))
    assert (cy.value, cb.value, ca.value) == (ny, nsb, nsa)
    ns = nsb if integrator == "baoab" else nsa

    y_tr, s_tr, x_tr = _Arena(ny, n, traj in ("all", "y")), _Arena(ns, n, traj == "all"), _Arena(ny, n, traj == "all")
    x_out = _Arena(1, n)
    y, v = y0.clone(), v0.clone()
    fn = smp._lib.jamun_walk_baoab if integrator == "baoab" else smp._lib.jamun_walk_aboba
    with torch.cuda.device(DEV):
        _lib.check(fn(smp._h, y.data_ptr(), v.data_ptr(), C.byref(params), None if noise is None else noise.data_ptr(), C.c_uint64(seed),
                      y_tr.ptr, s_tr.ptr, x_tr.ptr, x_out.ptr, int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for a in (y_tr, s_tr, x_tr, x_out):
        assert a.guards_untouched()

    yb, vb = y0.clone(), v0.clone()
    ref_y, ref_s = _reference_walk(integrator, smp, yb, vb, params, ref_noise, y_tr.passed)
    assert torch.equal(y, yb) and torch.equal(v, vb)
    if y_tr.passed:
        assert len(ref_y) == ny and _eq(y_tr.body(), ref_y)
    if s_tr.passed:
        assert len(ref_s) == ns and _eq(s_tr.body(), ref_s)
    if y_tr.passed and ny > 0 and ns > 0:  # where sampling._python_walk can express the case it is the same walk
        yc, vc = y0.clone(), v0.clone()
        py_y, py_s, _ = S._python_walk(integrator, yc, vc, lambda t: smp.score(t), params, ref_noise, 0, True)
        assert torch.equal(yc, y) and torch.equal(vc, v) and _eq(py_y, ref_y) and _eq(py_s, ref_s)
    if x_tr.passed:
        # x-hat of a saved frame is the denoiser at that frame's y.  BAOAB's saved scores are taken at the saved positions too, but the
        # initial score is kept even when burn-in drops frame 0: score_traj[t + 1] belongs to y_traj[t] then, score_traj[t] otherwise.
        shift = 0 if (burn_in <= 0) else 1
        for t in range(ny):
            assert torch.equal(x_tr.body()[t], smp.xhat(y_tr.body()[t])), t
            if integrator == "baoab":
                assert torch.equal(s_tr.body()[t + shift], smp.score(y_tr.body()[t])), t
        if integrator == "baoab":
            assert ns == ny + shift and torch.equal(s_tr.body()[0], smp.score(y0))
    assert torch.equal(x_out.body()[0], smp.xhat(y))
    norms = smp.score(y0).norm(dim=-1)
    if clip_kind == "binds":
        assert float((norms > clip).float().mean()) > 0.5  # the clip binds on more than half the rows
    elif clip_kind == "loose":
        assert bool((norms < clip).all()) and all(bool((s.norm(dim=-1) < clip).all()) for s in ref_s)
    assert torch.isfinite(y).all() and torch.isfinite(v).all()
    smp.check()


# ---- 3. the update kernels at their seams ---------------------------------------------------------------------------------------------

UPDATE_SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1025]


def _views(arrays, n, offset):
    """Device copies of [n, 3] arrays as views into larger allocations: at the allocation's start (16-byte aligned) or one atom
    (12 bytes) in, with a sentinel atom on either side."""
    out = []
    for a in arrays:
        base = torch.full((n + 4, 3), SENTINEL, device=DEV)
        view = base[offset : offset + n]
        view.copy_(torch.from_numpy(a))
        assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (offset == 0)
        out.append((base, view))
    return out


def _same(view, expected):
    return np.array_equal(view.cpu().numpy(), expected, equal_nan=True)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset12"])
@pytest.mark.parametrize("clip", [None, 3.0], ids=["noclip", "clip3"])
@pytest.mark.parametrize("n", UPDATE_SIZES)
def test_update_kernels_at_their_seams(n, clip, offset):
    """jamun_baoab_post (k_baoab_post4 for n / 4 groups on 16-byte-aligned buffers, k_baoab_post for the n % 4 remainder, and for
    everything on unaligned ones), jamun_baoab_pre, jamun_aboba_a and jamun_aboba_b against the formulas of include/jamun_hip.h in
    NumPy float32, one rounding per operation and no FMA except in the clip norm: bit-exact, and nothing outside the n atoms written."""
    from jamun_amd import native

    rng = np.random.RandomState(n + 7 * offset)
    y, v, psi, R = (rng.standard_normal((n, 3)).astype(np.float32) for _ in range(4))
    score = (5.0 * rng.standard_normal((n, 3))).astype(np.float32)
    delta, friction, M, beta = 0.05, 0.7, 2.0, 0.8
    params = native.make_mcmc_params(5, delta, friction, M, beta, clip)
    k = sc.langevin_consts(delta, friction, M)

    (bv, dv), (bp, dp), (bs, ds) = _views([v, psi, score], n, offset)
    native.baoab_post(dv, dp, ds, params)
    ev, ep = sc.np_baoab_post(v, score, k, beta, clip)
    assert _same(dv, ev) and _same(dp, ep) and _same(ds, score)
    for b in (bv, bp, bs):
        assert bool((b[:offset] == SENTINEL).all()) and bool((b[offset + n :] == SENTINEL).all())

    (by, dy), (bv, dv), (bp, dp), (bR, dR) = _views([y, v, psi, R], n, offset)
    native.baoab_pre(dy, dv, dp, dR, params)
    ey, ev = sc.np_baoab_pre(y, v, psi, R, k)
    assert _same(dy, ey) and _same(dv, ev) and _same(dp, psi)
    for b in (by, bv):
        assert bool((b[:offset] == SENTINEL).all()) and bool((b[offset + n :] == SENTINEL).all())

    (by, dy), (bv, dv) = _views([y, v], n, offset)
    native.aboba_a(dy, dv, params)
    assert _same(dy, sc.np_aboba_a(y, v, k)) and _same(dv, v)
    assert bool((by[:offset] == SENTINEL).all()) and bool((by[offset + n :] == SENTINEL).all())

    (by, dy), (bv, dv), (bs, ds), (bR, dR) = _views([y, v, score, R], n, offset)
    native.aboba_b(dy, dv, ds, dR, params)
    ey, ev = sc.np_aboba_b(y, v, score, R, k, beta, clip)
    assert _same(dy, ey) and _same(dv, ev)
    for b in (by, bv):
        assert bool((b[:offset] == SENTINEL).all()) and bool((b[offset + n :] == SENTINEL).all())
    if clip is not None and n >= 255:
        assert (np.linalg.norm(score, axis=1) > clip).mean() > 0.5  # the clip binds


@pytest.mark.parametrize("n,row", [(5, 4), (257, 100), (257, 256)])
def test_zero_score_row_under_a_clip_is_nan_in_that_row_only(n, row):
    """score / |score| of an all-zero row is 0 / 0: NaN in psi (and in what it updates) in that row and nowhere else — the behaviour of
    ``oracle.walk.process_score`` and of the reference's create_score_fn, pinned for the vector kernel, its remainder and k_aboba_b."""
    from jamun_amd import native

    rng = np.random.RandomState(n + row)
    y, v, R = (rng.standard_normal((n, 3)).astype(np.float32) for _ in range(3))
    score = (5.0 * rng.standard_normal((n, 3))).astype(np.float32)
    score[row] = 0.0
    params = native.make_mcmc_params(5, 0.05, 0.7, 2.0, 0.8, 3.0)
    k = sc.langevin_consts(0.05, 0.7, 2.0)
    only = [i == row for i in range(n)]
    (_, dv), (_, dp), (_, ds) = _views([v, np.zeros_like(v), score], n, 0)
    native.baoab_post(dv, dp, ds, params)
    ev, ep = sc.np_baoab_post(v, score, k, 0.8, 3.0)
    assert _same(dv, ev) and _same(dp, ep)
    assert torch.isnan(dp).all(dim=1).cpu().tolist() == only and torch.isnan(dv).all(dim=1).cpu().tolist() == only
    (_, dy), (_, dv), (_, ds), (_, dR) = _views([y, v, score, R], n, 0)
    native.aboba_b(dy, dv, ds, dR, params)
    ey, ev = sc.np_aboba_b(y, v, score, R, k, 0.8, 3.0)
    assert _same(dy, ey) and _same(dv, ev)
    assert torch.isnan(dy).all(dim=1).cpu().tolist() == only and torch.isnan(dv).any(dim=1).cpu().tolist() == only
