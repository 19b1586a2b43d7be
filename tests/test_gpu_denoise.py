"""GPU tests of the denoising evaluation: k_noise_align and k_denoise_loss (jamun_denoise.hip) through ``jamun_amd.native``, the
``Denoiser`` methods built on them, and ``denoise_eval.evaluate_denoiser``.  Expected values come from the host mirrors (bit for bit where
the kernel does the mirror's fp32 operations) and from the fp64 restatement of _denoise_cases.py, never from the GPU path itself;
test_denoise_host.py holds the premises (which graphs have a well-conditioned rotation, the mirrors against the restatement)."""
import json
import os

import numpy as np
import pytest
import torch

import _denoise_cases as dc
import _switch_cases as sc
from _denoise_cases import RMSD_TOL_NM

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = 2.0**-24


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _run(kind, sigma, **kw):
    from jamun_amd import native

    x, noise, ptr, _ = dc.batch(kind)
    x_c, y, r = native.noise_align_graphs(_t(x), _t(noise), torch.from_numpy(ptr.copy()), sigma, **kw)
    torch.cuda.synchronize()
    return x_c.cpu().numpy(), y.cpu().numpy(), r.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------------------- k_noise_align

@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_centring_and_noise_are_the_host_mirrors_bits(kind, sigma):
    """x_c is ``native.mean_center(x)`` bit for bit; without ``align`` y is the fp32 host mirror bit for bit, centring on and off; the RMSD
    of y to x_c comes with it."""
    from jamun_amd import native

    x, noise, ptr, _ = dc.batch(kind)
    for mean_center in (True, False):
        hx, hy, hr = native.noise_align_graphs_host(x, noise, ptr, sigma, mean_center=mean_center, align=False)
        gx, gy, gr = _run(kind, sigma, mean_center=mean_center, align=False)
        assert np.array_equal(gx, hx) and np.array_equal(gy, hy), mean_center
        assert np.abs(gr.astype(np.float64) - hr).max() <= RMSD_TOL_NM / 2
    centred = native.mean_center(_t(x), _t(ptr)).cpu().numpy()
    assert np.array_equal(_run(kind, sigma)[0], centred)


@pytest.mark.parametrize("mean_center", [True, False])
@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_aligned_y_against_the_fp64_kabsch_result(kind, sigma, mean_center):
    """Non-degenerate graphs: y within RMSD_TOL_NM per-graph RMSD of the fp64 Kabsch result and rmsd within half of it.  Degenerate graphs
    (one atom, two atoms, a line): finite, and the RMSD to x_c within RMSD_TOL_NM of the fp64 optimum, measured on the coordinates and as
    reported; their coordinates are not compared."""
    _, _, ptr, names = dc.batch(kind)
    x_c, y0, y_ref, rmsd_ref, _ = dc.aligned_case(kind, sigma, mean_center)
    gx, gy, gr = _run(kind, sigma, mean_center=mean_center, align=True)
    assert np.array_equal(gx, x_c) and np.isfinite(gy).all() and np.isfinite(gr).all()
    dev = dc.graph_rmsd(gy, y_ref, ptr)
    own = dc.graph_rmsd(gy, x_c, ptr)
    worst = [0.0, 0.0]
    for g, name in enumerate(names):
        if name in dc.DEGENERATE:
            assert abs(own[g] - rmsd_ref[g]) <= RMSD_TOL_NM and abs(float(gr[g]) - rmsd_ref[g]) <= RMSD_TOL_NM, name
        else:
            worst = [max(worst[0], dev[g]), max(worst[1], abs(float(gr[g]) - rmsd_ref[g]))]
            assert dev[g] <= RMSD_TOL_NM and abs(float(gr[g]) - rmsd_ref[g]) <= RMSD_TOL_NM / 2, (name, dev[g], gr[g], rmsd_ref[g])
    print(f"{kind} sigma {sigma} mean_center {mean_center}: coordinates {worst[0]:.2e} nm, rmsd {worst[1]:.2e} nm from the fp64 result")


@pytest.mark.parametrize("which", list(dc.SPECIAL_SIGNS))
def test_identity_half_turns_and_the_mirror_image(which):
    """y equal to x: unchanged within the bound.  y a half turn of x: recovered.  y the exact mirror image of x: a proper rotation (the
    pairwise distances of y survive), rmsd > 0 and equal to the fp64 value."""
    from jamun_amd import native

    x, noise, ptr, y0 = dc.special_case(which)
    gx, gy, gr = native.noise_align_graphs(_t(x), _t(noise), _t(ptr), dc.SPECIAL_SIGMA, mean_center=False, align=True)
    _, g0, _ = native.noise_align_graphs(_t(x), _t(noise), _t(ptr), dc.SPECIAL_SIGMA, mean_center=False, align=False)
    gx, gy, gr, g0 = gx.cpu().numpy(), gy.cpu().numpy(), gr.cpu().numpy(), g0.cpu().numpy()
    assert np.array_equal(gx, x) and np.array_equal(g0, y0)
    y_ref = dc.kabsch_reference(y0, x, ptr)
    rmsd_ref = dc.graph_rmsd(y_ref, x, ptr)
    assert dc.graph_rmsd(gy, y_ref, ptr).max() <= RMSD_TOL_NM
    assert np.abs(gr.astype(np.float64) - rmsd_ref).max() <= RMSD_TOL_NM / 2
    if which == "mirror":
        assert gr.min() > 100 * RMSD_TOL_NM
        for _, lo, hi in dc.graphs(ptr):  # rotated, not reflected: every distance of y is kept, and the handedness with them
            d_out = np.linalg.norm(gy[lo:hi, None].astype(np.float64) - gy[None, lo:hi], axis=-1)
            d_in = np.linalg.norm(y0[lo:hi, None].astype(np.float64) - y0[None, lo:hi], axis=-1)
            assert np.abs(d_out - d_in).max() <= 10 * RMSD_TOL_NM
            a, b = gy[lo : lo + 4].astype(np.float64), y0[lo : lo + 4].astype(np.float64)
            assert np.sign(np.linalg.det(a[1:] - a[0])) == np.sign(np.linalg.det(b[1:] - b[0]))
    else:
        assert dc.graph_rmsd(gy, x, ptr).max() <= RMSD_TOL_NM and gr.max() <= RMSD_TOL_NM


def test_a_nan_atom_spoils_its_graph_only_two_runs_agree_and_empty_graphs_write_nothing():
    from jamun_amd import native

    x, noise, ptr, names = dc.batch("ragged")
    tx, tp = _t(x), _t(ptr)
    clean = native.noise_align_graphs(tx, _t(noise), tp, 0.04)
    again = native.noise_align_graphs(tx, _t(noise), tp, 0.04)
    assert all(torch.equal(a, b) for a, b in zip(clean, again))
    bad = noise.copy()
    g_bad = names.index("chain64")
    bad[ptr[g_bad] + 5, 1] = np.nan
    spoiled = native.noise_align_graphs(tx, _t(bad), tp, 0.04)
    torch.cuda.synchronize()
    for g, lo, hi in dc.graphs(ptr):
        if g == g_bad:
            assert not torch.isfinite(spoiled[1][lo:hi]).any() and not torch.isfinite(spoiled[2][g])
            assert torch.equal(spoiled[0][lo:hi], clean[0][lo:hi])  # (x is clean: so is x_c)
        else:
            assert torch.equal(spoiled[1][lo:hi], clean[1][lo:hi]) and torch.equal(spoiled[2][g], clean[2][g])
    # graphs without atoms, in the middle and at the end: the others' bits, nothing written behind the last atom
    lo17, hi17 = int(ptr[2]), int(ptr[3])
    N = hi17 - lo17
    sentinel = 777.0
    big_y = torch.full((N + 8, 3), sentinel, device=DEV)
    ptr2 = torch.tensor([0, 0, N, N, N])
    xs, ns = tx[lo17:hi17].contiguous(), _t(noise)[lo17:hi17].contiguous()
    _, y2, r2 = native.noise_align_graphs(xs, ns, ptr2, 0.04, out_y=big_y[:N])
    torch.cuda.synchronize()
    assert torch.equal(y2, clean[1][lo17:hi17]) and (big_y[N:] == sentinel).all()
    assert r2.tolist() == [0.0, float(clean[2][2]), 0.0, 0.0]
    loss = native.denoise_loss(y2, xs, ptr2, 0.04, 1.0).cpu().numpy()
    assert not loss[0].any() and not loss[2:].any() and (loss[1] > 0).all()


def test_a_side_stream_behind_its_producer_gives_the_default_streams_bits():
    from jamun_amd import native

    x, noise, ptr, _ = dc.batch("dense")
    tn, tp = _t(noise), _t(ptr)
    ref = native.noise_align_graphs(_t(x), tn, tp, 0.04)
    ref_loss = native.denoise_loss(ref[1], ref[0], tp, 0.04, 2.5)
    torch.cuda.synchronize()
    half = _t(x * np.float32(0.5))
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        tx = half + half  # the producer of x, on the side stream: exact, x again
        got = native.noise_align_graphs(tx, tn, tp, 0.04)
        got_loss = native.denoise_loss(got[1], got[0], tp, 0.04, 2.5)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ref, got)) and torch.equal(ref_loss, got_loss)


# -------------------------------------------------------------------------------------------------------------------------- k_denoise_loss

@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_losses_within_the_bound_of_a_sequential_fp32_sum(kind, sigma):
    """Each of the three outputs within (n + 4) 2^-24 relative of the fp64 value — the bound of a sequential fp32 sum of n non-negative
    terms plus the per-term roundings; derived, not measured — and equal to the host mirror, which does the same operations.  A null
    loss_weight is a weight of ones."""
    from jamun_amd import native

    _, _, ptr, _ = dc.batch(kind)
    x_c, y0, *_ = dc.aligned_case(kind, sigma)
    W = len(ptr) - 1
    lw = (1.0 + np.arange(W) / W).astype(np.float32)
    inv = float(np.float32(7.25))
    ref = dc.loss_reference(y0, x_c, ptr, sigma, lw, inv)
    tp = _t(ptr)
    got = native.denoise_loss(_t(y0), _t(x_c), tp, sigma, inv, _t(lw)).cpu().numpy()
    n = np.diff(ptr)[:, None]
    rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    print(f"{kind} sigma {sigma}: worst error over bound {(rel / ((n + 4) * U)).max():.3f}")
    assert (rel <= (n + 4) * U).all()  # (chain1 is centred on its only atom: every value 0, and 0 is what comes back)
    assert np.array_equal(got, native.denoise_loss_host(y0, x_c, ptr, sigma, inv, lw))
    ones = native.denoise_loss(_t(y0), _t(x_c), tp, sigma, inv, torch.ones(W, device=DEV))
    assert torch.equal(native.denoise_loss(_t(y0), _t(x_c), tp, sigma, inv), ones)


# ------------------------------------------------------------------------------------------------------------------------------ end to end

_models = {}


def _model():
    from jamun_amd.model import Denoiser

    if "m" not in _models:
        _models["ck"] = sc.checkpoint()
        _models["m"] = Denoiser.from_checkpoint_dict(_models["ck"]).to(DEV)
    return _models["m"], _models["ck"]


@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.E2E))
def test_noise_and_denoise_and_the_losses_against_the_fp64_oracle(kind, sigma):
    """``rng="torch_cpu"``: the noise is the global CPU generator's next draw, so the test knows it.  x-hat within 1e-5 nm per-graph RMSD of
    the fp64 oracle fed the GPU's own y (y is held to its reference above, so it is an input here); scaled_rmsd within 1e-5 / (sigma sqrt 3)
    of the fp64 value from the oracle's x-hat (the mean of norms moves by at most the RMSD); the other two within the same relative share."""
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch
    from oracle import denoiser as od

    model, ck = _model()
    mols = dc.E2E[kind]()
    g = torch.Generator().manual_seed(5)
    mols = [dict(m, pos=m["pos"] + 0.02 * torch.randn(m["pos"].shape, generator=g)) for m in mols]  # every walker its own frame
    x = WalkerBatch.from_molecules(mols).to(DEV)
    ptr = x.ptr.cpu().numpy()
    torch.manual_seed(17)
    noise = torch.randn(x.pos.shape)
    torch.manual_seed(17)
    xhat, y = model.noise_and_denoise(x, sigma, align_noisy_input=True, rng="torch_cpu")
    # y is what the kernel makes of x and that draw
    x_c, y_mine, _ = native.noise_align_graphs(x.pos, noise.to(DEV), x.ptr, sigma)
    assert torch.equal(y.pos, y_mine) and xhat.topology_id == x.topology_id
    topo, p, hp = sc.oracle_setup(mols, ck, torch.float64)
    x_ref = od.xhat(y.pos.cpu().double(), topo, sigma, p, hp).numpy()
    dev = dc.graph_rmsd(xhat.pos.cpu().numpy(), x_ref, ptr)
    print(f"{kind} sigma {sigma}: x-hat within {dev.max():.2e} nm of the fp64 oracle")
    assert dev.max() <= RMSD_TOL_NM
    k = float(model.loss_weight(sigma, model.average_squared_distance))
    ref = dc.loss_reference(x_ref, x_c.cpu().numpy(), ptr, sigma, None, k)
    loss, aux = model.compute_loss(x, xhat, sigma)
    torch.manual_seed(17)
    loss2, aux2 = model.noise_and_compute_loss(x, sigma, align_noisy_input=True, rng="torch_cpu")
    assert torch.equal(loss, aux["coordinate_loss"]) and all(torch.equal(aux[m], aux2[m]) for m in aux) and torch.equal(loss, loss2)
    tol = RMSD_TOL_NM / (float(np.float32(sigma)) * np.sqrt(3.0))
    got = aux["scaled_rmsd"].cpu().numpy().astype(np.float64)
    print(f"{kind} sigma {sigma}: scaled_rmsd {got.mean():.4f}, within {np.abs(got - ref[:, 1]).max():.2e} of the fp64 value (bound {tol:.2e})")
    assert np.abs(got - ref[:, 1]).max() <= tol
    # raw = mean |d|^2: |d| moves by at most the RMSD bound per graph in the root-mean-square sense
    raw = aux["raw_coordinate_loss"].cpu().numpy().astype(np.float64)
    assert (np.abs(np.sqrt(raw) - np.sqrt(ref[:, 0])) <= RMSD_TOL_NM).all()
    assert np.allclose(aux["coordinate_loss"].cpu().numpy(), raw * k, rtol=4 * U)
    # add_noise: x + sigma noise, no centring, no mirror
    torch.manual_seed(17)
    assert torch.equal(model.add_noise(x, sigma, rng="torch_cpu").pos, x.pos + torch.tensor(sigma, dtype=torch.float32) * noise.to(DEV))


def test_evaluate_denoiser_reproduces_batch_by_batch_calls(tmp_path):
    """12 frames, batch_size 8: one full and one short batch per sigma.  The per-frame columns are those of `noise_and_compute_loss`
    called batch by batch under the same seed."""
    from jamun_amd import denoise_eval, synth
    from jamun_amd.data import WalkerBatch

    model, _ = _model()
    ds = dc.FramesDataset(synth.random_chain(17, seed=0), "chain17", 12)
    out = str(tmp_path / "denoise")
    res = denoise_eval.evaluate_denoiser(model, [ds], list(dc.SIGMAS), batch_size=8, align_noisy_input=True, seed=23, rng="torch_cpu", output_dir=out)
    z = np.load(os.path.join(out, "chain17.npz"))
    torch.manual_seed(23)
    for si, sigma in enumerate(dc.SIGMAS):
        for lo, hi in ((0, 8), (8, 12)):
            x = WalkerBatch.from_molecules([ds[i] for i in range(lo, hi)]).to(DEV)
            _, aux = model.noise_and_compute_loss(x, sigma, align_noisy_input=True, rng="torch_cpu")
            for m in denoise_eval.METRICS:
                assert np.array_equal(z[m][si, lo:hi], aux[m].cpu().numpy()), (m, sigma, lo)
        assert res[f"chain17/scaled_rmsd_per_dataset/sigma={sigma}"] == float(z["scaled_rmsd"][si].astype(np.float64).mean())
    assert json.load(open(os.path.join(out, "summary.json")))["metrics"] == res


def test_quick_start_command_from_a_pdb_and_a_checkpoint_to_summary_json(tmp_path, monkeypatch):
    from jamun_amd import denoise_eval, pdb, synth

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mol = dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)
    pdb_path = str(tmp_path / "uncapped_AG.pdb")
    pdb.write_pdb(pdb_path, mol, mol["pos"][None])
    (tmp_path / "ckpt").mkdir()
    torch.save(synth.synthetic_checkpoint(output_gain=0.05), str(tmp_path / "ckpt" / "last.ckpt"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("JAMUN_ROOT_PATH", str(tmp_path))
    run_dir = denoise_eval.main(["--config-dir=" + os.path.join(root, "configs"), "experiment=sample_custom", f"++init_pdbs=[{pdb_path}]",
                                 "++checkpoint_dir=ckpt", "++sigma_list=[0.04,0.1]", "++num_frames=1", "++align_noisy_input=true"])
    summary = json.load(open(os.path.join(run_dir, "denoise", "summary.json")))
    assert sorted(summary["metrics"]) == sorted(f"uncapped_AG/{m}_per_dataset/sigma={s}" for m in denoise_eval.METRICS for s in (0.04, 0.1))
    assert all(np.isfinite(v) and v > 0 for v in summary["metrics"].values())
    assert np.load(os.path.join(run_dir, "denoise", "uncapped_AG.npz"))["scaled_rmsd"].shape == (2, 1)
