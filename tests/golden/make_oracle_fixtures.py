"""Cache CPU-oracle outputs for the GPU parity tests (the oracle needs minutes of CPU time; GPU-minutes are scarce).

    python tests/golden/make_oracle_fixtures.py

Inputs are generated from fixed seeds with ``jamun_amd.synth``; outputs come from ``oracle/``.
``tests/test_oracle.py::test_cached_oracle_fixtures_are_fresh`` re-runs a prefix of each case on the CPU and checks
the cache bit for bit, so a stale cache cannot go unnoticed.  Both run under PINNED_ENV (``main`` starts itself again under it):
one thread, MKL's conditional numerical reproducibility and ATen's generic kernels give the same bits on any x86 CPU, where the
default thread count and instruction-set dispatch would make the cache depend on the machine that wrote it.
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from jamun_amd import synth  # noqa: E402
from oracle import denoiser as od  # noqa: E402
from oracle import graph as og  # noqa: E402
from oracle import walk as ow  # noqa: E402

SIGMA = 0.04
MCMC = dict(delta=0.04, friction=1.0, M=1.0, inverse_temperature=1.0, score_fn_clip=100.0, save_trajectory=True)
# "strong": O(1) activations, stresses kernel numerics in one forward.  "stable": small output gain, contractive
# dynamics, so that fp32 rounding differences are not amplified exponentially along a trajectory.
# Measured (tests/test_oracle.py::test_fp32_oracle_leaves_fp64_trajectory, AG x 4, 50 steps): gains 0.05 and 0.1 are contractive
# (fp32 vs fp64 oracle stay at 2e-8 .. 7e-8 nm for all 50 frames); 0.2 and 0.5 are chaotic (1.5e-5 / 5.8e-5 nm at step 21,
# 5e-2 / 2e-1 nm at step 49).
GAINS = {"strong": 0.5, "stable": 0.05, "mid": 0.1, "g02": 0.2}
PINNED_ENV = {"OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1", "MKL_CBWR": "COMPATIBLE,STRICT", "ATEN_CPU_CAPABILITY": "default"}


def molecules(kind):
    if kind == "ag4":
        return [synth.ag_dipeptide()] * 4
    if kind == "ag32":
        return [synth.ag_dipeptide()] * 32
    if kind == "chain17x6":
        return [synth.random_chain(17, seed=0)] * 6
    if kind == "ragged":
        return [synth.random_chain(n, seed=s) for s, n in enumerate([5, 17, 33, 9, 57, 2, 1, 29])]
    if kind == "dense70":
        return [synth.random_chain(70, seed=3, bond=0.12, min_dist=0.13)] * 2
    # BASELINE configs[4] sizes: chignolin with hydrogens (~166 atoms) and H-stripped as the reference feeds it to the model
    # (93 heavy atoms, src/jamun/data/_mdtraj.py:60,218).  44 % / 8 % of the atoms hit torch_cluster's 32-neighbour cap.
    if kind == "chig93x2":
        return [synth.random_chain(93, seed=5)] * 2
    if kind == "chig166x2":
        return [synth.random_chain(166, seed=5)] * 2
    # per-GPU shapes of BASELINE configs[2] / configs[3] (bench.py cfg3 / cfg4): the 33-atom molecule of the 4AA workload, and
    # the eight distinct sequences (17..57 atoms) of the ragged MDGen-like batch — embedded into full-size batches by
    # tests/test_gpu_parity.py::test_full_size_batches_of_the_multi_gpu_configs_match_the_oracle
    if kind == "chain33x4":
        return [synth.random_chain(33, seed=0)] * 4
    # BASELINE configs[1] as the reference runs it (sample_uncapped_2AA.yaml:18-19): one walker per distinct dipeptide — 48 of the 400,
    # real topology (9..29 heavy atoms), every residue type: 100+ distinct embedding rows in one batch
    if kind == "dipep48":
        codes = synth.all_dipeptides()
        return [synth.peptide(codes[(i * 400) // 48 + (i % 7)], seed=i) for i in range(48)]
    if kind == "cfg4kinds":
        import random

        rng = random.Random(1234)
        return [synth.random_chain(rng.randint(17, 57), seed=100 + i) for i in range(8)]
    # large molecules of mixed sizes in one batch (5AA-like peptides with hydrogens, 63..120 atoms; analysis/sampling_times/JAMUN.csv:6) next to
    # small ones: tile spans of one and of two molecules, windows starting at odd atoms — the tile plan of jamun_conv_ml.hip
    if kind == "large_mix":
        return [synth.random_chain(n, seed=40 + i) for i, n in enumerate([63, 9, 101, 64, 120, 3, 77])]
    raise KeyError(kind)


# Hyper-parameter points / architectures / weight distributions beyond the default one, each with the reference file that ships it
# ("A, sigma and max_radius are per-checkpoint values, never hard-code").  `ckpt`: keyword arguments of
# jamun_amd.synth.synthetic_checkpoint; `sigma`: the noise level of the forward.
VARIANTS = {
    "default": dict(ckpt={}, sigma=SIGMA),
    # configs/experiment/train_test.yaml:7-8 (n_layers: 2)
    "nl2": dict(ckpt=dict(arch=synth.default_arch(n_layers=2)), sigma=SIGMA),
    # hydra_config/model/arch/e3conv_separable.yaml:6 (SeparableConv, n_layers: 4)
    "sep_nl4": dict(ckpt=dict(arch=synth.default_arch(n_layers=4), separable=True), sigma=SIGMA),
    # configs/experiment/train_idrome_cg.yaml:13-17 (sigma 0.25, max_radius 6.0, average_squared_distance 9.5): on nm-scale
    # molecules every atom of a molecule above 33 atoms sits at the 32-neighbour cap and the radial basis is far below its first centre
    "idrome": dict(ckpt=dict(max_radius=6.0, average_squared_distance=9.5), sigma=0.25),
    # configs/experiment/train_test_single_shape.yaml:9 (max_radius: 1000)
    "r1000": dict(ckpt=dict(max_radius=1000.0), sigma=SIGMA),
    # a narrower hidden representation than e3conv.yaml's 120x0e + 32x1e
    "h64x16": dict(ckpt=dict(arch=synth.default_arch(irreps_hidden="64x0e + 16x1e")), sigma=SIGMA),
    # "trained-like" weights (synth.trained_like: per-channel scale spread 2^+-10, 1 % outliers x 100), a second seed
    "trained": dict(ckpt=dict(weights="trained_like", seed=1), sigma=SIGMA),
    "sep_trained": dict(ckpt=dict(weights="trained_like", seed=1, separable=True), sigma=SIGMA),
}


def variant_checkpoint(variant, output_gain=GAINS["strong"]):
    return synth.synthetic_checkpoint(output_gain=output_gain, **VARIANTS[variant]["ckpt"])


def variant_hparams(ckpt):
    hp = ckpt["hyper_parameters"]
    arch = {k: v for k, v in hp["arch"].items() if k != "hidden_layer_factory"}
    return od.default_hparams(max_radius=hp["max_radius"], average_squared_distance=hp["average_squared_distance"],
                              conv="separable" if "hidden_layer_factory" in hp["arch"] else "conv", **arch)


def setup(kind, preset, dtype=torch.float32, separable=False, variant=None):
    mols = molecules(kind)
    topo = og.collate([{k: v for k, v in m.items() if torch.is_tensor(v)} for m in mols])
    if variant is not None:
        ck = variant_checkpoint(variant, GAINS[preset])
        return mols, topo, {k[2:]: v.to(dtype) for k, v in ck["state_dict"].items()}, variant_hparams(ck)
    sd = synth.synthetic_state_dict(output_gain=GAINS[preset], separable=separable)
    p = {k: v.to(dtype) for k, v in sd.items()}
    return mols, topo, p, od.default_hparams(conv="separable" if separable else "conv")


def forward_case(kind, with_layers, separable=False, variant=None):
    mols, topo, p, hp = setup(kind, "strong", separable=separable, variant=variant)
    sigma = VARIANTS[variant]["sigma"] if variant else SIGMA
    torch.manual_seed(2)
    y = topo["pos"] + sigma * torch.randn_like(topo["pos"])
    x, inter = od.xhat(y, topo, sigma, p, hp, return_intermediates=True)
    s = od.score(y, topo, sigma, p, hp)
    out = dict(y=y, xhat=x, score=s, g=inter["g"], deg=torch.bincount(inter["edge_index"][1], minlength=y.shape[0]),
               n_edges=torch.tensor(inter["edge_index"].shape[1]))
    if with_layers:
        for l in range(hp["n_layers"] + 1):
            out[f"x{l}"] = inter[f"x{l}"]
    return out


def walk_case(kind, integrator, steps, preset, max_steps=None, variant=None):
    mols, topo, p, hp = setup(kind, preset, variant=variant)
    g = torch.Generator().manual_seed(42)
    noise = torch.randn(steps + 1, topo["pos"].shape[0], 3, generator=g)
    run_steps = steps if max_steps is None else min(steps, max_steps)
    rec = ow.RecordedNoise(noise)
    y0 = topo["pos"] + rec(topo["pos"]) * SIGMA
    out = ow.walk_jump(lambda y: od.score(y, topo, SIGMA, p, hp), lambda y: od.xhat(y, topo, SIGMA, p, hp),
                       getattr(ow, integrator), y0, "gaussian", rec, steps=run_steps, **MCMC)
    res = dict(noise=noise, y0=y0)
    res.update({k: v for k, v in out.items() if torch.is_tensor(v)})
    return res


def sampler_case(continue_chain, steps=8, num_batches=2, max_batches=None):
    mols, topo, p, hp = setup("ag4", "stable")
    nb = num_batches if max_batches is None else min(num_batches, max_batches)
    outs = ow.sampler_loop(topo["pos"], lambda y: od.score(y, topo, SIGMA, p, hp), lambda y: od.xhat(y, topo, SIGMA, p, hp), ow.baoab,
                           SIGMA, nb, continue_chain, ow.TorchNoise(42), steps=steps, **MCMC)
    return {f"xhat_traj_{b}": o["xhat_traj"] for b, o in enumerate(outs)} | {f"y_{b}": o["y"] for b, o in enumerate(outs)}


# ---- the command-line runs of tests/test_gpu_cli.py, end to end -------------------------------------------------------
# The oracle is fed from the source of truth, not from the product's readers (a reader bug must not cancel out): topology tensors from
# jamun_amd.synth, positions from the file on disk through the few lines below, parameters restated from the experiment yaml.
CLI_PARAMS = dict(delta=0.05, friction=0.7, M=1.3, inverse_temperature=0.9, score_fn_clip=40.0, save_trajectory=True)
CLI_PARAMS_SEED = 7
# score_fn_clip = 40 binds on some atoms and not on others: measured in the oracle run (2 x 12 steps, 40 atoms; stored as `clip_share`,
# asserted in tests/test_cli_cases_host.py) 0.384 of the per-atom score norms are above it.  The norms have two sources: the noise,
# about chi_3 / sigma = 25 chi_3 (median 38), and on the first steps the centroid of the file's coordinates, which x-hat removes and y
# keeps (0.35 nm / sigma^2 = 220).  A clip of 0.5 or 3 binds on every atom (share 1: indistinguishable from a fixed step length).
# the dipeptides of test_jamun_sample_uncapped_2aa_directory_end_to_end in the order the test lists them (the seed of a code is its place here)
CLI_2AA_CODES = ["AG", "GG", "WW", "FY", "KR", "PH", "CM", "DE", "NQ", "ST", "IL", "VA", "RK", "HP", "MC", "ED", "QN", "TS", "LI", "YF",
                 "GW", "WA", "AV", "SG", "PP", "KE", "DR", "HH"]


def pdb_heavy_positions_nm(path):
    """Decimal columns 31-54 of the ATOM records of the first model, Angstrom / 10 as float32, and which records are not hydrogens
    (element columns 77-78)."""
    xyz, heavy = [], []
    for line in open(path):
        if line.startswith("ENDMDL"):
            break
        if line.startswith("ATOM  "):
            xyz.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
            heavy.append(line[76:78].strip() != "H")
    return torch.from_numpy(np.asarray(xyz, dtype=np.float32) / np.float32(10.0)), np.asarray(heavy)


def _topology(mol):
    return {k: v for k, v in mol.items() if torch.is_tensor(v) and k != "pos"}


def cli_oracle_run(mols, seed, steps, num_batches, mcmc, max_steps=None, max_batches=None):
    """`sampler_loop` over the collated molecules with the stable checkpoint, TorchNoise(seed) and continue_chain, as `jamun_sample` runs
    it; returns the inputs the oracle consumed, per batch xhat_traj / y, and the share of per-atom score norms above the clip."""
    topo = og.collate(mols)
    p = {k: v.to(torch.float32) for k, v in synth.synthetic_state_dict(output_gain=GAINS["stable"]).items()}
    hp = od.default_hparams()
    steps = steps if max_steps is None else min(steps, max_steps)
    nb = num_batches if max_batches is None else min(num_batches, max_batches)
    norms = []

    def score_fn(y):
        s = od.score(y, topo, SIGMA, p, hp)
        norms.append(torch.linalg.vector_norm(s, dim=-1))
        return s

    outs = ow.sampler_loop(topo["pos"], score_fn, lambda y: od.xhat(y, topo, SIGMA, p, hp), ow.baoab, SIGMA, nb, True, ow.TorchNoise(seed),
                           steps=steps, **mcmc)
    res = {k: topo[k] for k in ("pos", "atom_type_index", "atom_code_index", "residue_code_index", "residue_sequence_index", "bonds", "ptr")}
    res["clip_share"] = (torch.cat(norms) > mcmc["score_fn_clip"]).float().mean()
    for b, o in enumerate(outs):
        res[f"xhat_traj_{b}"], res[f"y_{b}"] = o["xhat_traj"], o["y"]
    return res


def cli_cfg1_case(mcmc, seed, steps, max_steps=None, max_batches=None):
    """`jamun_sample experiment=sample_custom ++init_pdbs=[uncapped_AG.pdb] repeat_init_samples=4 num_batches=2` on the AG dipeptide
    file as tests/test_gpu_cli.py writes it."""
    import tempfile

    from jamun_amd import pdb

    mol = dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "uncapped_AG.pdb")
        pdb.write_pdb(path, mol, mol["pos"][None])
        pos, heavy = pdb_heavy_positions_nm(path)
    assert heavy.all() and pos.shape == mol["pos"].shape
    return cli_oracle_run([dict(_topology(synth.ag_dipeptide()), pos=pos)] * 4, seed, steps, 2, mcmc, max_steps, max_batches)


def cli_2aa_case(steps=12, max_steps=None, max_batches=None):
    """`jamun_sample experiment=sample_timewarp_2AA ++init_datasets.num_frames=1` over the 28-code tree of tests/test_gpu_cli.py: one walker
    per code in sorted order (the reference sorts the codes of a directory, data/_utils.py:94), each at frame 0 of its `positions`."""
    import tempfile

    mols = []
    order = sorted(CLI_2AA_CODES)
    with tempfile.TemporaryDirectory() as d:
        synth.write_timewarp_tree(d, CLI_2AA_CODES, n_frames=2)
        for code in order:
            top = _topology(synth.peptide(code, seed=CLI_2AA_CODES.index(code)))
            _, heavy = pdb_heavy_positions_nm(os.path.join(d, f"{code}-traj-state0.pdb"))
            frame0 = np.load(os.path.join(d, f"{code}-traj-arrays.npz"))["positions"][0]
            assert frame0.dtype == np.float32 and frame0.shape[0] == heavy.shape[0] and int(heavy.sum()) == top["atom_type_index"].shape[0]
            mols.append(dict(top, pos=torch.from_numpy(frame0[heavy].copy())))
    res = cli_oracle_run(mols, 42, steps, 2, MCMC, max_steps, max_batches)
    res["codes"] = torch.tensor([[ord(c) for c in code] for code in order], dtype=torch.uint8)  # the walkers' labels, in batch order
    return res


CASES = {
    "oracle_cli_cfg1": lambda max_steps=None, max_batches=None, **kw: cli_cfg1_case(MCMC, 42, 50, max_steps, max_batches),
    "oracle_cli_cfg1_params": lambda max_steps=None, max_batches=None, **kw: cli_cfg1_case(CLI_PARAMS, CLI_PARAMS_SEED, 12, max_steps, max_batches),
    "oracle_cli_2aa": lambda max_steps=None, max_batches=None, **kw: cli_2aa_case(12, max_steps, max_batches),
    "oracle_forward_ag4": lambda **kw: forward_case("ag4", True),
    "oracle_forward_chain17x6": lambda **kw: forward_case("chain17x6", True),
    "oracle_forward_ragged": lambda **kw: forward_case("ragged", False),
    "oracle_forward_dense70": lambda **kw: forward_case("dense70", False),
    "oracle_forward_chig93x2": lambda **kw: forward_case("chig93x2", False),
    "oracle_forward_chig166x2": lambda **kw: forward_case("chig166x2", False),
    "oracle_forward_chain33x4": lambda **kw: forward_case("chain33x4", False),
    # SeparableConv architecture (hydra_config/model/arch/e3conv_separable.yaml): small, ragged, chignolin-size
    "oracle_forward_sep_ag4": lambda **kw: forward_case("ag4", True, separable=True),
    "oracle_forward_sep_ragged": lambda **kw: forward_case("ragged", False, separable=True),
    "oracle_forward_sep_chig93x2": lambda **kw: forward_case("chig93x2", False, separable=True),
    "oracle_forward_cfg4kinds": lambda **kw: forward_case("cfg4kinds", False),
    # beyond the default hyper-parameter point / architecture / weight distribution (VARIANTS above)
    "oracle_forward_dipep48": lambda **kw: forward_case("dipep48", True),
    "oracle_forward_nl2_ragged": lambda **kw: forward_case("ragged", True, variant="nl2"),
    "oracle_forward_sep_nl4_ragged": lambda **kw: forward_case("ragged", True, variant="sep_nl4"),
    "oracle_forward_idrome_ragged": lambda **kw: forward_case("ragged", True, variant="idrome"),
    "oracle_forward_idrome_dense70": lambda **kw: forward_case("dense70", False, variant="idrome"),
    "oracle_forward_r1000_ragged": lambda **kw: forward_case("ragged", True, variant="r1000"),
    "oracle_forward_h64x16_ragged": lambda **kw: forward_case("ragged", True, variant="h64x16"),
    "oracle_forward_trained_chain17x6": lambda **kw: forward_case("chain17x6", True, variant="trained"),
    "oracle_forward_trained_ragged": lambda **kw: forward_case("ragged", True, variant="trained"),
    "oracle_forward_trained_chig93x2": lambda **kw: forward_case("chig93x2", True, variant="trained"),
    "oracle_forward_large_mix": lambda **kw: forward_case("large_mix", True),
    "oracle_forward_sep_trained_ragged": lambda **kw: forward_case("ragged", True, variant="sep_trained"),
    "oracle_walk_baoab_trained_ag4_12": lambda max_steps=None, **kw: walk_case("ag4", "baoab", 12, "stable", max_steps, variant="trained"),
    "oracle_walk_baoab_trained_chig93_6": lambda max_steps=None, **kw: walk_case("chig93x2", "baoab", 6, "stable", max_steps, variant="trained"),
    "oracle_walk_baoab_chig93_6": lambda max_steps=None, **kw: walk_case("chig93x2", "baoab", 6, "stable", max_steps),
    "oracle_walk_baoab_chig166_4": lambda max_steps=None, **kw: walk_case("chig166x2", "baoab", 4, "stable", max_steps),
    "oracle_walk_baoab_ag4_50_mid": lambda max_steps=None, **kw: walk_case("ag4", "baoab", 50, "mid", max_steps),
    "oracle_walk_baoab_ag4_50_g02": lambda max_steps=None, **kw: walk_case("ag4", "baoab", 50, "g02", max_steps),
    "oracle_walk_baoab_ag4_50": lambda max_steps=None, **kw: walk_case("ag4", "baoab", 50, "stable", max_steps),
    "oracle_walk_baoab_ag4_20_strong": lambda max_steps=None, **kw: walk_case("ag4", "baoab", 20, "strong", max_steps),
    # a LONG walk with the strongly non-linear checkpoint (the bench checkpoint's gain): single trajectories leave the oracle's after ~40
    # steps — what must still agree is the ENSEMBLE (tests/test_gpu_variants.py: statistics of frames 40..80)
    "oracle_walk_baoab_ag32_80_strong": lambda max_steps=None, **kw: walk_case("ag32", "baoab", 80, "strong", max_steps),
    "oracle_walk_baoab_ragged_12": lambda max_steps=None, **kw: walk_case("ragged", "baoab", 12, "stable", max_steps),
    "oracle_walk_aboba_ag4_20": lambda max_steps=None, **kw: walk_case("ag4", "aboba", 20, "stable", max_steps),
    "oracle_sampler_cc1": lambda max_batches=None, **kw: sampler_case(True, max_batches=max_batches),
    "oracle_sampler_cc0": lambda max_batches=None, **kw: sampler_case(False, max_batches=max_batches),
}


def main():
    if any(os.environ.get(k) != v for k, v in PINNED_ENV.items()):  # (read when torch and MKL start: a child process of its own)
        raise SystemExit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(os.environ, **PINNED_ENV)))
    torch.set_num_threads(1)
    only = set(sys.argv[1:])
    for name, fn in CASES.items():
        if only and name not in only:
            continue
        out = fn()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **{k: v.numpy() for k, v in out.items()})
        print(name, {k: tuple(v.shape) for k, v in out.items()}, flush=True)


if __name__ == "__main__":
    main()
