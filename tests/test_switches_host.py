"""CPU-side premises of ``test_gpu_switches.py`` (no GPU): what the oracle itself does under the checkpoint / sampling switches.

* the oracle's ``w3j_111_sign``: +1 is bit-identical to the cached fixtures, -1 is the reflection conjugate of +1;
* every switch changes x-hat on the chosen inputs by at least 100 tolerances (so a GPU path that ignored it could not pass);
* the fp32 CPU oracle against the fp64 oracle under per-walker translations (``mean_center = False``) and over the noise levels — the
  reference's own share of every bound the GPU test uses;
* the reference's frame-count rule against ``jamun_num_frames`` (host-only code of the library), and the walk table's pair coverage;
* the NumPy restatement of the update kernels against ``oracle.walk.process_score``.
"""
import ctypes as C
import importlib.util
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _switch_cases as sc
from oracle import denoiser as od
from oracle import walk as ow

HERE = os.path.dirname(os.path.abspath(__file__))


def _xhat(mols, ck, y=None, dtype=torch.float64, sigma=sc.SIGMA, **kw):
    topo, p, hp = sc.oracle_setup(mols, ck, dtype)
    if y is None:
        y = sc.noisy_positions(topo, sigma)
    return od.xhat(y.to(dtype), topo, sigma, p, hp, **kw)


# ---- 0. the sign of wigner_3j(1, 1, 1) in the oracle ---------------------------------------------------------------------------------


def test_oracle_with_the_default_sign_is_bit_identical_to_the_cached_fixture(golden_dir, tmp_path):
    """``default_hparams`` carries ``w3j_111_sign = +1.0`` and +1 leaves the (1, 1, 1) tensor untouched: the AG forward, run under the
    generator's pinned environment, reproduces the cached fixture bit for bit (x-hat, score, the last block's features)."""
    assert od.default_hparams()["w3j_111_sign"] == 1.0
    path = os.path.join(golden_dir, "make_oracle_fixtures.py")
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    code = ("import importlib.util, sys\nimport numpy as np, torch\ntorch.set_num_threads(1)\n"
            "spec = importlib.util.spec_from_file_location('mk', sys.argv[1]); mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)\n"
            "assert mk.od.default_hparams()['w3j_111_sign'] == 1.0\n"
            "f = mk.forward_case('ag4', True)\n"
            "np.savez(sys.argv[2], **{k: f[k].numpy() for k in ('xhat', 'score', 'x5')})\n")
    r = subprocess.run([sys.executable, "-c", code, path, str(tmp_path / "fresh.npz")], env=dict(os.environ, **mk.PINNED_ENV),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    fresh, cached = np.load(tmp_path / "fresh.npz"), np.load(os.path.join(golden_dir, "oracle_forward_ag4.npz"))
    for k in ("xhat", "score", "x5"):
        assert np.array_equal(fresh[k], cached[k]), k


@pytest.mark.parametrize("separable", [False, True], ids=["conv", "separable"])
def test_oracle_with_the_opposite_sign_is_the_reflection_conjugate(separable):
    """xhat_{-1}(y) = -xhat_{+1}(-y), exactly.  Derivation: let P negate every coordinate.  The graph of -y is the graph of y (distances,
    centring and the neighbour order are unchanged), the radial features are unchanged, and Y_1 changes sign.  Claim: with the sign of
    the (1, 1, 1) tensor flipped as well, every scalar feature is unchanged and every vector feature negated, block by block — the
    embedding is scalar; 0e x Y_0 -> 0e is unchanged; 0e x Y_1 -> 1e is negated by Y_1; 1e x Y_0 -> 1e is negated by the input;
    1e . Y_1 -> 0e is a product of two negated factors; s (1e x Y_1) -> 1e has three negated factors (s, the input, Y_1); gates are
    scalars; o3.Linear does not mix l.  So g_{-1}(-y) = -g_{+1}(y) and, x-hat being c_skip y + c_out g (centred or not),
    xhat_{-1}(-y) = -xhat_{+1}(y).  Negation is exact in floating point and the summation orders are the same on both sides, so the
    fp64 runs agree to rounding (asserted 1e-12 nm).  The flipped sign alone moves x-hat by more than 100 tolerances."""
    mols = sc.molecules("chain17x6")
    plus, minus = sc.checkpoint(separable=separable), sc.checkpoint(separable=separable, w3j_111_sign=-1.0)
    topo, _, hp_minus = sc.oracle_setup(mols, minus)
    assert hp_minus["w3j_111_sign"] == -1.0 and sc.oracle_setup(mols, plus)[2]["w3j_111_sign"] == 1.0
    y = sc.noisy_positions(topo, sc.SIGMA).double()
    x_minus = _xhat(mols, minus, y)
    assert (x_minus + _xhat(mols, plus, -y)).abs().max().item() <= 1e-12
    assert sc.rmsd(x_minus, _xhat(mols, plus, y)) >= sc.DID_SOMETHING


# ---- 1. premises of the denoiser switches --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["chain17x6", "ragged", "chig93x2"])
def test_translated_input_without_centring_premises(kind):
    """``mean_center = False`` with one 8 nm translation per walker: the fp32 CPU oracle stays within a quarter of the tolerance
    (2.5e-6 nm RMSD) of the fp64 oracle, the two build the same edges, centring on / off differ by more than 100 tolerances, and the
    oracle's response to a coordinate perturbation stays below the gain the translation law's bound assumes.
    Measured (fp32 against fp64, nm RMSD) at 0.5 / 2 / 8 nm:  chain17x6 8.0e-8 / 1.9e-7 / 6.8e-7;  ragged 1.1e-7 / 2.0e-7 / 6.9e-7;
    chig93x2 1.1e-7 / 2.0e-7 / 6.5e-7 — 8 nm, the largest of the three sizes, qualifies on every set.  Gain (max |delta x-hat - c_skip
    delta| / max |delta| for a random 1e-7 nm perturbation): 2.1, 15.8, 1.8."""
    assert sc.TRANSLATION_NM == max(sc.TRANSLATION_SIZES_NM)
    mols, ck = sc.molecules(kind), sc.checkpoint(mean_center=False)
    topo, p64, hp = sc.oracle_setup(mols, ck)
    assert hp["mean_center"] is False
    y = sc.noisy_positions(topo, sc.SIGMA) + sc.walker_translations(topo["num_graphs"], sc.TRANSLATION_NM, topo["batch"])
    x64, i64 = od.xhat(y.double(), topo, sc.SIGMA, p64, hp, return_intermediates=True)
    x32, i32 = _xhat(mols, ck, y, torch.float32, return_intermediates=True)
    dev = sc.rmsd(x32, x64)
    print(f"{kind}: fp32 oracle against fp64 at {sc.TRANSLATION_NM} nm: {dev:.3e} nm")
    assert dev <= sc.REF_SHARE_NM, dev
    assert torch.equal(i32["edge_index"], i64["edge_index"])
    assert sc.rmsd(x64, _xhat(mols, sc.checkpoint(mean_center=True), y)) >= sc.DID_SOMETHING
    g = torch.Generator().manual_seed(1)
    d = (torch.rand(y.shape, generator=g, dtype=torch.float64) * 2 - 1) * 1e-7
    gain = ((od.xhat(y.double() + d, topo, sc.SIGMA, p64, hp) - x64 - float(sc.c_skip_fp32(sc.SIGMA)) * d).abs().max() / d.abs().max()).item()
    print(f"{kind}: response gain {gain:.2f}")
    assert gain <= sc.TRANSLATION_LAW_GAIN, gain


@pytest.mark.parametrize("kind,rows_off,rows_on", [("chain17x6", 16, 16), ("ragged50", 105, 105), ("chain17_shifted", 16, 48)])
def test_sequence_index_premises(kind, rows_off, rows_on):
    """The sets of the sequence-index test: their distinct embedding rows lie on both sides of 32 (one set crosses it with the switch),
    every index fits the 10-row table, and the switch moves the oracle's x-hat by more than 100 tolerances."""
    mols = sc.molecules(kind)
    assert (sc.embedding_rows(mols, False), sc.embedding_rows(mols, True)) == (rows_off, rows_on)
    assert max(int(m["residue_sequence_index"].max()) for m in mols) <= 9
    on, off = sc.checkpoint(use_residue_sequence_index=True), sc.checkpoint()
    assert sc.oracle_setup(mols, on)[2]["use_residue_sequence_index"] is True
    assert sc.rmsd(_xhat(mols, on), _xhat(mols, off)) >= sc.DID_SOMETHING
    assert int(sc.synth.random_chain(57, seed=4)["residue_sequence_index"].max()) == 11  # the negative case: outside the table


@pytest.mark.parametrize("kind", ["chain17x6", "ragged"])
def test_sign_premise_on_the_default_architecture(kind):
    mols = sc.molecules(kind)
    assert sc.rmsd(_xhat(mols, sc.checkpoint(w3j_111_sign=-1.0)), _xhat(mols, sc.checkpoint())) >= sc.DID_SOMETHING


@pytest.mark.parametrize("kind", ["ragged", "dense70"])
def test_fp32_oracle_against_fp64_over_the_noise_levels(kind):
    """The reference's own error at sigma 0.01 / 0.1 / 0.4 / 1.0 (c_out and the cutoff grow with sigma).  Measured nm RMSD:
    ragged 3.5e-8 / 1.5e-7 / 4.2e-7 / 3.9e-7;  dense70 3.7e-8 / 8.7e-8 / 2.8e-7 / 3.6e-7 — all within a quarter of the tolerance, so the
    GPU bound is the project's 1e-5 nm at every level (``sc.xhat_bound``); the two precisions build the same edges, and neighbouring
    noise levels differ by more than 100 tolerances (the level does something)."""
    mols, ck = sc.molecules(kind), sc.checkpoint()
    topo = sc.oracle_setup(mols, ck)[0]
    prev = None
    for sigma in sc.SIGMAS:
        y = sc.noisy_positions(topo, sigma)
        x64, i64 = _xhat(mols, ck, y, sigma=sigma, return_intermediates=True)
        x32, i32 = _xhat(mols, ck, y, torch.float32, sigma=sigma, return_intermediates=True)
        dev = sc.rmsd(x32, x64)
        print(f"{kind} sigma {sigma}: fp32 oracle against fp64 {dev:.3e} nm, bound {sc.xhat_bound(kind, sigma):.1e}")
        assert dev <= 2 * sc.SIGMA_REF_DEV_NM[kind][sigma] and dev <= sc.REF_SHARE_NM, (sigma, dev)
        assert torch.equal(i32["edge_index"], i64["edge_index"])
        if prev is not None:
            assert sc.rmsd(x64, _xhat(mols, ck, y, sigma=prev)) >= sc.DID_SOMETHING
        prev = sigma
    if kind == "dense70":
        assert int(torch.bincount(i64["edge_index"][1]).max()) >= 32  # the neighbour cap binds


def test_xhat_bound_rule():
    assert sc.xhat_bound_from(2.5e-6) == 1e-5 and sc.xhat_bound_from(1e-9) == 1e-5 and sc.xhat_bound_from(5e-6) == 2e-5


# ---- 2. the walk grid -----------------------------------------------------------------------------------------------------------------


def test_frame_counts_of_the_reference_rule_equal_jamun_num_frames():
    """``jamun_num_frames`` is host-only code of the library: against the reference's rule restated in three lines
    (``reference_frame_counts``) for every (steps, save_every, burn_in) the walk table can reach and around it."""
    from jamun_amd import _lib, native

    lib = _lib.load()
    n = 0
    for steps in range(1, 13):
        for save_every in range(1, steps + 7):
            for burn_in in range(0, steps + 3):
                p = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, None, save_every, burn_in)
                ny, nb, na = C.c_int32(), C.c_int32(), C.c_int32()
                _lib.check(lib.jamun_num_frames(C.byref(p), C.byref(ny), C.byref(nb), C.byref(na)))
                assert (ny.value, nb.value, na.value) == sc.reference_frame_counts(steps, save_every, burn_in), (steps, save_every, burn_in)
                n += 1
    assert n > 1000
    assert sc.reference_frame_counts(9, 2, 3) == (3, 4, 3)  # baoab_clip_mass-like: frames 4, 6, 8 and the initial score
    assert sc.reference_frame_counts(3, 1, 3) == (0, 1, 0) and sc.reference_frame_counts(1, 1, 0) == (1, 1, 0)


def test_walk_table_covers_every_pair_of_axis_values():
    cases = sc.WALK_CASES
    assert len(set(cases)) == len(cases) and 50 <= len(cases) <= 70
    for c in cases:
        assert len(c) == len(sc.WALK_AXES) and all(v in axis for v, axis in zip(c, sc.WALK_AXES)), c
        assert c[1] <= 10 and (c[7] != "big" or c[1] <= 3), c
    for i, j in itertools.combinations(range(len(sc.WALK_AXES)), 2):
        for a, b in itertools.product(sc.WALK_AXES[i], sc.WALK_AXES[j]):
            if (i, j) == (1, 7) and b == "big" and a > 3:
                continue  # (the 1100-atom batch walks at most 3 steps)
            assert any(c[i] == a and c[j] == b for c in cases), (i, a, j, b)
    totals = {k: sum(v) % 4 for k, v in sc.WALK_BATCHES.items()}
    assert [totals[k] for k in ("m0", "m1", "m2", "m3")] == [0, 1, 2, 3] and max(sc.WALK_BATCHES["big"]) > 1024


# ---- 3. the NumPy restatement of the update kernels ---------------------------------------------------------------------------------


@pytest.mark.parametrize("clip", [None, 3.0, 1e6])
def test_numpy_process_score_equals_the_oracle(clip):
    """``np_process_score`` (what the update-kernel tests compare the HIP kernels with) against ``oracle.walk.process_score``, bit for
    bit on the CPU — including the all-zero row, which gives NaN under a clip and only there."""
    g = torch.Generator().manual_seed(0)
    s = 5.0 * torch.randn(257, 3, generator=g)
    s[100] = 0.0
    ref = ow.process_score(s, 0.8, clip)[0].numpy()
    out = sc.np_process_score(s.numpy(), 0.8, clip)
    assert np.array_equal(out, ref, equal_nan=True)
    assert np.isnan(out).any(axis=1).tolist() == [clip is not None and i == 100 for i in range(257)]


@pytest.mark.parametrize("clip", [None, 3.0])
def test_numpy_update_formulas_equal_the_oracle_integrators(clip):
    """The NumPy float32 restatement composed into whole BAOAB / ABOBA walks against ``oracle.walk.baoab`` / ``aboba`` (pinned to the
    reference's own goldens in test_oracle.py) on the same noise and a closed-form score, bit for bit.  Parameters are dyadic so that
    their fp32 and double forms are the same numbers."""
    steps, delta, friction, M, beta = 5, 0.0625, 0.75, 2.0, 0.75
    g = torch.Generator().manual_seed(3)
    y0, v0 = torch.randn(37, 3, generator=g), torch.randn(37, 3, generator=g)
    noise = torch.randn(steps - 1, 37, 3, generator=g)
    score_fn = lambda t: -40.0 * t + 3.0 * torch.sin(5.0 * t)  # noqa: E731
    kw = dict(steps=steps, delta=delta, friction=friction, M=M, inverse_temperature=beta, score_fn_clip=clip, v_init=v0)
    k = sc.langevin_consts(delta, friction, M)
    score = lambda a: score_fn(torch.from_numpy(a)).numpy()  # noqa: E731

    yb, vb, _, _ = ow.baoab(y0, score_fn, noise=ow.RecordedNoise(noise), **kw)
    y, v = y0.numpy().copy(), v0.numpy().copy()
    psi = sc.np_process_score(score(y), beta, clip)
    for i in range(1, steps):
        y, v = sc.np_baoab_pre(y, v, psi, noise[i - 1].numpy(), k)
        v, psi = sc.np_baoab_post(v, score(y), k, beta, clip)
    assert np.array_equal(y, yb.numpy()) and np.array_equal(v, vb.numpy())

    ya, va, _, _ = ow.aboba(y0, score_fn, noise=ow.RecordedNoise(noise), save_trajectory=True, **kw)
    y, v = y0.numpy().copy(), v0.numpy().copy()
    for i in range(1, steps):
        y = sc.np_aboba_a(y, v, k)
        y, v = sc.np_aboba_b(y, v, score(y), noise[i - 1].numpy(), k, beta, clip)
    assert np.array_equal(y, ya.numpy()) and np.array_equal(v, va.numpy())
