"""GPU parity of the wide path (``jamun_wide.hip``; ``-m gpu``): Conv models outside the compiled-width kernels' envelope — wider hidden
irreps, channel counts that are not multiples of 4 or 32, other radial sizes (odd ones included), a 256-wide embedding, shallow networks —
against the CPU oracle, evaluated here on the same inputs.  Tolerances of ``test_gpu_variants.py``: x-hat <= 1e-5 nm RMSD, score
<= 1e-5 / sigma^2, per-block features <= 2e-5 of the block maximum, degree and edge count exact."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RMSD_TOL_NM = 1e-5
SIGMA = 0.04
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _mk():
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", os.path.join(HERE, "golden", "make_oracle_fixtures.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def rmsd(a, b):
    return ((a.double().cpu() - b.double().cpu()) ** 2).sum(-1).mean().sqrt().item()


def _checkpoint(arch_over, weights="gaussian", gain=0.5):
    from jamun_amd import synth

    return synth.synthetic_checkpoint(arch=synth.default_arch(**arch_over), output_gain=gain, weights=weights)


def _oracle(mk, ck, kind):
    from oracle import denoiser as od
    from oracle import graph as og

    mols = mk.molecules(kind)
    topo = og.collate([{k: v for k, v in m.items() if torch.is_tensor(v)} for m in mols])
    p = {k[2:]: v for k, v in ck["state_dict"].items()}
    hp = mk.variant_hparams(ck)
    torch.manual_seed(2)
    y = topo["pos"] + SIGMA * torch.randn_like(topo["pos"])
    x, inter = od.xhat(y, topo, SIGMA, p, hp, return_intermediates=True)
    return mols, y, x, inter, hp


def _sampler(ck, mols):
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    dev = torch.device("cuda", 0)
    model = Denoiser.from_checkpoint_dict(ck).to(dev)
    return model.sampler_for(WalkerBatch.from_molecules(mols).to(dev), SIGMA)


def _assert_wide(st):
    assert (st["conv_path"], st["init_path"], st["dg_mode"], st["dg_emu"]) == (3, 6, -1, 0), st


CASES = [
    ("h160x48", dict(irreps_hidden="160x0e + 48x1e"), "ag4", "gaussian"),
    ("h256x64", dict(irreps_hidden="256x0e + 64x1e"), "ag4", "gaussian"),
    ("h150x37", dict(irreps_hidden="150x0e + 37x1e"), "ag4", "gaussian"),
    ("H32", dict(edge_attr_dim=32), "ag4", "gaussian"),
    ("H33", dict(edge_attr_dim=33), "ragged", "gaussian"),
    ("H128", dict(edge_attr_dim=128), "ag4", "gaussian"),
    ("emb256", dict(atom_type_embedding_dim=32, atom_code_embedding_dim=32, residue_code_embedding_dim=160, residue_index_embedding_dim=32), "ag4", "gaussian"),
    ("nl1", dict(irreps_hidden="160x0e + 48x1e", n_layers=1), "ag4", "gaussian"),
    ("nl0", dict(irreps_hidden="160x0e + 48x1e", n_layers=0), "ag4", "gaussian"),
    ("trained256x64", dict(irreps_hidden="256x0e + 64x1e"), "ag4", "trained_like"),
]


@pytest.mark.parametrize("name,over,kind,weights", CASES, ids=[c[0] for c in CASES])
def test_wide_forward_matches_oracle(name, over, kind, weights):
    mk = _mk()
    ck = _checkpoint(over, weights)
    mols, y, x_ref, inter, hp = _oracle(mk, ck, kind)
    smp = _sampler(ck, mols)
    dev = torch.device("cuda", 0)
    x = smp.xhat(y.to(dev))
    st = smp.stats()
    _assert_wide(st)
    deg = torch.bincount(inter["edge_index"][1], minlength=y.shape[0])
    assert torch.equal(smp.debug_read(1).cpu().flatten().long(), deg)
    assert st["n_edges"] == inter["edge_index"].shape[1]
    for l in range(hp["n_layers"] + 1):
        xl, r = smp.debug_read(0, l).cpu(), inter[f"x{l}"]
        err = (xl - r).abs().max().item() / max(r.abs().max().item(), 1e-6)
        assert err < 2e-5, (l, err)
        if weights == "trained_like":  # per channel, as test_gpu_variants.py: the channels spread over 2^+-10
            cmax = r.abs().amax(0)
            cerr = ((xl - r).abs().amax(0) / cmax.clamp_min(1e-30)).max().item()
            assert cerr < 1e-4, (l, cerr)
    g = smp.debug_read(2).cpu()
    assert (g - inter["g"]).abs().max().item() < 2e-5 * max(inter["g"].abs().max().item(), 1.0)
    assert rmsd(x, x_ref) <= RMSD_TOL_NM, rmsd(x, x_ref)
    s = smp.score(y.to(dev))
    assert rmsd(s, (x_ref - y) / SIGMA**2) <= RMSD_TOL_NM / SIGMA**2


def test_wide_forward_is_bit_reproducible_and_conv_block_matches_the_forward():
    mk = _mk()
    ck = _checkpoint(dict(irreps_hidden="150x0e + 37x1e", edge_attr_dim=33))
    mols = mk.molecules("ragged")
    smp = _sampler(ck, mols)
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    pos = torch.cat([m["pos"] for m in mols])
    y = (pos + SIGMA * torch.randn_like(pos)).to(dev)
    a = smp.xhat(y).clone()
    feats = [smp.debug_read(0, l).clone() for l in range(ck["hyper_parameters"]["arch"]["n_layers"] + 1)]
    b = smp.xhat(y).clone()
    assert torch.equal(a, b)
    _assert_wide(smp.stats())
    smp.build_edges(y)
    assert torch.equal(smp.conv_block(0), feats[0])
    for l in range(1, len(feats)):
        assert torch.equal(smp.conv_block(l, feats[l - 1]), feats[l]), l


def test_wide_baoab_walk_matches_the_oracle_walk():
    from jamun_amd import native
    from oracle import denoiser as od
    from oracle import graph as og
    from oracle import walk as ow

    mk = _mk()
    ck = _checkpoint(dict(irreps_hidden="256x0e + 64x1e"), gain=mk.GAINS["stable"])
    mols = mk.molecules("ag4")
    smp = _sampler(ck, mols)
    dev = torch.device("cuda", 0)
    steps = 12
    g = torch.Generator().manual_seed(42)
    topo = og.collate([{k: t for k, t in m.items() if torch.is_tensor(t)} for m in mols])
    noise = torch.randn(steps + 1, topo["pos"].shape[0], 3, generator=g)
    y0 = topo["pos"] + SIGMA * noise[0]
    params = native.make_mcmc_params(steps, 0.04, 1.0, 1.0, 1.0, 100.0)
    y, v = y0.to(dev).clone(), noise[1].to(dev).clone()
    y_traj, score_traj, xhat_traj, xhat = smp.walk("baoab", y, v, params, noise[2 : steps + 1].to(dev).contiguous(), 0, True)
    torch.cuda.synchronize()
    _assert_wide(smp.stats())
    p = {k[2:]: t for k, t in ck["state_dict"].items()}
    hp = mk.variant_hparams(ck)
    ref = ow.walk_jump(lambda t: od.score(t, topo, SIGMA, p, hp), lambda t: od.xhat(t, topo, SIGMA, p, hp), ow.baoab, y0, noise[1],
                       ow.RecordedNoise(noise[2:]), steps=steps, delta=0.04, friction=1.0, M=1.0, inverse_temperature=1.0,
                       score_fn_clip=100.0, save_trajectory=True)
    assert xhat_traj.shape == ref["xhat_traj"].shape
    for f in range(xhat_traj.shape[0]):
        assert rmsd(xhat_traj[f], ref["xhat_traj"][f]) <= RMSD_TOL_NM, (f, rmsd(xhat_traj[f], ref["xhat_traj"][f]))


def test_wide_checkpoint_samples_through_the_python_sampler_and_the_cli(tmp_path, monkeypatch):
    from jamun_amd import cmdline, pdb, synth

    ck = synth.synthetic_checkpoint(arch=synth.default_arch(irreps_hidden="256x0e + 64x1e", edge_attr_dim=33), output_gain=0.05,
                                    prefix="g._orig_mod.")
    from jamun_amd.data import WalkerBatch
    from jamun_amd.model import Denoiser

    dev = torch.device("cuda", 0)
    model = Denoiser.from_checkpoint_dict(ck).to(dev)
    batch = WalkerBatch.from_molecules([synth.ag_dipeptide()] * 4).to(dev)
    _assert_wide(model.sampler_for(batch, SIGMA).stats())
    # the command line: checkpoint file -> Denoiser -> Sampler.sample -> trajectory callbacks

    mol = dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)
    pdb_path = str(tmp_path / "uncapped_AG.pdb")
    pdb.write_pdb(pdb_path, mol, mol["pos"][None])
    ck_dir = tmp_path / "ckpt"
    ck_dir.mkdir()
    torch.save(ck, str(ck_dir / "epoch=7-step=100.ckpt"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("JAMUN_ROOT_PATH", str(tmp_path))
    run_dir = cmdline.main(["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", f"++init_pdbs=[{pdb_path}]",
                            f"++checkpoint_dir={ck_dir}", "checkpoint_type=best_so_far", "wandb_train_run_path=null", "finetune_on_init=null",
                            "num_sampling_steps_per_batch=20", "repeat_init_samples=4", "num_batches=1", "++sampler.rng=torch_cpu"])
    npy = os.path.join(run_dir, "sampler", "uncapped_AG", "predicted_samples", "npy")
    chains = [np.load(os.path.join(npy, f"{i}.npy")) for i in range(4)]
    assert all(c.shape == (10, 20, 3) and np.isfinite(c).all() for c in chains)
    assert np.abs(chains[0] - chains[1]).max() > 1e-3 and np.abs(chains[0]).max() < 5.0
    assert os.path.exists(os.path.join(run_dir, "sampler", "uncapped_AG", "predicted_samples", "pdb", "joined.pdb"))
