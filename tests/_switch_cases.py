"""Cases and restatements shared by ``test_switches_host.py`` (CPU) and ``test_gpu_switches.py`` (GPU): the checkpoint / sampling
switches a user's files set — ``mean_center``, ``use_residue_sequence_index``, the sign of ``wigner_3j(1, 1, 1)``, the noise level — and
the parameter grid of the fused walks.  The host file asserts the premises of every bound on the CPU oracle; the GPU file holds the HIP
path to those bounds."""
import math

import numpy as np
import torch

from jamun_amd import synth

RMSD_TOL_NM = 1e-5  # the project's x-hat tolerance (BASELINE.json north star: 1e-4 Angstrom)
DID_SOMETHING = 100 * RMSD_TOL_NM  # "the switch did something": on and off differ by at least 100 tolerances
REF_SHARE_NM = RMSD_TOL_NM / 4  # what the fp32 CPU oracle may spend of the tolerance on an input (the kernel keeps three quarters)
SIGMA = 0.04
TRANSLATION_SIZES_NM = (0.5, 2.0, 8.0)
TRANSLATION_NM = 8.0  # the largest of TRANSLATION_SIZES_NM at which the fp32 oracle stays inside REF_SHARE_NM (test_switches_host.py)
SIGMAS = (0.01, 0.1, 0.4, 1.0)
# fp32 CPU oracle against the fp64 oracle, nm RMSD, per molecule set and noise level: measured on the CPU (test_switches_host.py asserts
# that the oracle stays within twice these — its summation order moves with the machine's thread count — and inside REF_SHARE_NM)
SIGMA_REF_DEV_NM = {"ragged": {0.01: 3.5e-8, 0.1: 1.5e-7, 0.4: 4.2e-7, 1.0: 3.9e-7}, "dense70": {0.01: 3.7e-8, 0.1: 8.7e-8, 0.4: 2.8e-7, 1.0: 3.7e-7}}
# the translation law xhat(y + t) - xhat(y) = c_skip t holds to TRANSLATION_LAW_K * eps32 * max |y + t|:
#   2    four roundings of c_skip * y + c_out * g on the two sides, half an ulp of the translated magnitude at most each;
#   1.5  the perturbation of the geometry in units of eps32 |y + t| per coordinate: 0.5 for the rounding of y + t itself, 1 for the
#        difference of two scaled coordinates c_in q - c_in p (two products of half an ulp each), ...
#   x 20 ... times the response of c_out g to a coordinate perturbation, max |delta x-hat - c_skip delta| / max |delta|, which the
#        fp64 CPU oracle keeps below TRANSLATION_LAW_GAIN on these inputs (test_switches_host.py: measured 2.1, 15.8, 1.8)
TRANSLATION_LAW_GAIN = 20.0
TRANSLATION_LAW_K = 2.0 + 1.5 * TRANSLATION_LAW_GAIN
EPS32 = 2.0**-23


def xhat_bound_from(reference_deviation_nm):
    """The GPU's x-hat bound at a noise level from the reference's own fp32 error there: the project's 1e-5 nm where the fp32 oracle
    spends at most a quarter of it, four times the oracle's deviation where it spends more."""
    return RMSD_TOL_NM if reference_deviation_nm <= REF_SHARE_NM else 4.0 * reference_deviation_nm


def xhat_bound(kind, sigma):
    return xhat_bound_from(SIGMA_REF_DEV_NM[kind][sigma])


def rmsd(a, b):
    return ((a.double().cpu() - b.double().cpu()) ** 2).sum(-1).mean().sqrt().item()


def shifted_sequence(mol: dict, offset: int) -> dict:
    """The molecule with ``offset`` added to every residue sequence index (a fragment cut out of a longer chain)."""
    return dict(mol, residue_sequence_index=mol["residue_sequence_index"] + offset)


def molecules(kind):
    """The molecule sets of tests/golden/make_oracle_fixtures.py that the switch tests use, plus the ones only they need."""
    if kind == "chain17x6":
        return [synth.random_chain(17, seed=0)] * 6
    if kind == "ragged":
        return [synth.random_chain(n, seed=s) for s, n in enumerate([5, 17, 33, 9, 57, 2, 1, 29])]
    if kind == "chain33x4":
        return [synth.random_chain(33, seed=0)] * 4
    if kind == "dense70":
        return [synth.random_chain(70, seed=3, bond=0.12, min_dist=0.13)] * 2
    if kind == "chig93x2":
        return [synth.random_chain(93, seed=5)] * 2
    if kind == "big1100":  # test_geometry_of_a_molecule_above_the_lds_budget_of_k_geom: one molecule above GEOM_LDS_ATOMS (1024)
        big, small = synth.random_chain(1100, seed=7, min_dist=0.2), synth.random_chain(17, seed=8)
        return [small, big, small]
    # ``ragged`` with every molecule at most 50 atoms: synth.random_chain numbers residues idx // 5 and the index table has 10 rows
    if kind == "ragged50":
        return [synth.random_chain(n, seed=s) for s, n in enumerate([5, 17, 33, 9, 50, 2, 1, 29])]
    # three fragments of one 17-atom chain at sequence offsets 0, 3, 6: the same 17 embedding rows without the sequence index, three times
    # as many with it — the two sides of the 32-row limit between the initial projectors k_conv_mfi and k_conv_mfx
    if kind == "chain17_shifted":
        return [shifted_sequence(synth.random_chain(17, seed=0), o) for o in (0, 3, 6)]
    raise KeyError(kind)


def checkpoint(gain=0.5, mean_center=True, use_residue_sequence_index=False, w3j_111_sign=1.0, separable=False, arch_over=None):
    """``synth.synthetic_checkpoint`` edited the way a user's checkpoint would differ: ``mean_center`` in the hyper-parameters,
    ``use_residue_sequence_index`` in the architecture, and the sign of wigner_3j(1, 1, 1) as the e3nn buffers ``_w3j_1_1_1`` of the
    tensor products in the state dict (``checkpoint.w3j_111_sign_from_state_dict`` reads them)."""
    arch = synth.default_arch(**dict(arch_over or {}, use_residue_sequence_index=bool(use_residue_sequence_index)))
    ck = synth.synthetic_checkpoint(arch=arch, output_gain=gain, separable=separable)
    ck["hyper_parameters"]["mean_center"] = bool(mean_center)
    if w3j_111_sign != 1.0:
        eps = torch.zeros(3, 3, 3)
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            eps[i, j, k], eps[i, k, j] = 1.0, -1.0
        for l in range(arch["n_layers"]):
            ck["state_dict"][f"g.layers.{l}.gated_conv.f.f.tp._w3j_1_1_1"] = float(w3j_111_sign) * eps / math.sqrt(6.0)
    return ck


def collate(mols):
    from oracle import graph as og

    return og.collate([{k: v for k, v in m.items() if torch.is_tensor(v)} for m in mols])


def oracle_setup(mols, ck, dtype=torch.float64):
    """(topology, parameters in ``dtype``, oracle hyper-parameters) of a checkpoint dict — the switches read as the loader reads them."""
    from jamun_amd.checkpoint import w3j_111_sign_from_state_dict
    from oracle import denoiser as od

    topo = collate(mols)
    p = {k[2:]: v.to(dtype) for k, v in ck["state_dict"].items() if "_w3j_" not in k}
    hpar = ck["hyper_parameters"]
    arch = {k: v for k, v in hpar["arch"].items() if k != "hidden_layer_factory"}
    hp = od.default_hparams(max_radius=hpar["max_radius"], average_squared_distance=hpar["average_squared_distance"],
                            mean_center=hpar["mean_center"], conv="separable" if "hidden_layer_factory" in hpar["arch"] else "conv",
                            w3j_111_sign=w3j_111_sign_from_state_dict(ck["state_dict"]), **arch)
    return topo, p, hp


def noisy_positions(topo, sigma, seed=11):
    g = torch.Generator().manual_seed(seed)
    return topo["pos"] + sigma * torch.randn(topo["pos"].shape, generator=g)


def walker_translations(n_graphs, size_nm, batch):
    """One translation per walker, each of length ``size_nm`` in its own direction, as a per-atom fp32 tensor."""
    g = torch.Generator().manual_seed(7)
    d = torch.randn(n_graphs, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True) * size_nm
    return d.float()[batch]


def c_skip_fp32(sigma, average_squared_distance=0.332):
    """c_skip as jamun_sampler_create computes it, op for op in fp32: A / (A + 6 (sigma sigma))."""
    f = np.float32
    A, B = f(average_squared_distance), f(6.0) * (f(sigma) * f(sigma))
    return A / (A + B)


def embedding_rows(mols, use_sequence_index):
    """Distinct (atom type, atom code, residue, sequence index) tuples of a batch — the sequence index reads 0 when the switch is off."""
    rows = set()
    for m in mols:
        seq = m["residue_sequence_index"].tolist() if use_sequence_index else [0] * m["pos"].shape[0]
        rows |= set(zip(m["atom_type_index"].tolist(), m["atom_code_index"].tolist(), m["residue_code_index"].tolist(), seq))
    return len(rows)


def expected_init_path(mols, use_sequence_index):
    """k_conv_mfi (3) up to 32 distinct embedding rows, k_conv_mfx (4) above (on the tiles of k_conv_mf)."""
    return 3 if embedding_rows(mols, use_sequence_index) <= 32 else 4


# ---- the walk grid -------------------------------------------------------------------------------------------------------------------

def reference_frame_counts(steps, save_every, burn_in):
    """The reference's rule (functional/_splitting.py:70-72,99-101,138-140,168-170), restated: frame i of range(steps) is kept when
    i % save_every == 0 and i >= burn_in; BAOAB always keeps the initial score, ABOBA has no score at i = 0."""
    kept = [i for i in range(steps) if i % save_every == 0 and i >= burn_in]
    later = sum(1 for i in kept if i >= 1)
    return len(kept), 1 + later, later  # y frames, BAOAB score frames, ABOBA score frames


def save_and_burn(code, steps):
    """(save_every_n_steps, burn_in_steps) of a table entry: "1,S" burns in all ``steps`` (no y frame at all), "S+5,0" saves every
    ``steps + 5`` (frame 0 only)."""
    return {"1,0": (1, 0), "3,0": (3, 0), "2,3": (2, 3), "1,S": (1, steps), "S+5,0": (steps + 5, 0)}[code]


WALK_BATCHES = {  # atoms of each walker; the totals are 0, 1, 2, 3 modulo 4, and one batch holds a molecule above 1024 atoms
    "m0": [17, 17, 2], "m1": [17, 9, 7], "m2": [17, 17], "m3": [17, 5, 1], "big": [17, 1100, 17],
}
MCMC = {"unit": (1.0, 1.0, 1.0), "heavy": (2.0, 0.7, 0.8)}  # M, friction, inverse temperature
CLIP_BINDS, CLIP_LOOSE = 3.0, 1e6


def walk_molecules(name):
    return [synth.random_chain(n, seed=20 + i, **({"min_dist": 0.2} if n > 1024 else {})) for i, n in enumerate(WALK_BATCHES[name])]


# (integrator, steps, (save_every, burn_in) code, clip, noise, trajectory pointers, no_fuse_geom, batch, mean_center, M / friction / beta):
# two greedy pairwise coverings of the axes' values (every pair of values of two axes occurs; the 1100-atom batch walks at most 3 steps),
# written out so that what runs can be read here.  tests/test_switches_host.py checks the covering.
WALK_CASES = [
    ('baoab', 1, '1,0', 'binds', 'tensor', 'all', 0, 'big', False, 'unit'),
    ('baoab', 1, '1,0', 'loose', 'seed', 'none', 1, 'm1', True, 'heavy'),
    ('baoab', 1, '1,0', 'none', 'tensor', 'all', 0, 'm3', False, 'unit'),
    ('baoab', 1, '2,3', 'binds', 'seed', 'none', 1, 'm1', False, 'unit'),
    ('baoab', 1, '2,3', 'binds', 'tensor', 'none', 1, 'm0', True, 'unit'),
    ('baoab', 1, '3,0', 'binds', 'tensor', 'all', 0, 'm0', True, 'unit'),
    ('baoab', 1, '3,0', 'loose', 'seed', 'y', 0, 'm2', False, 'unit'),
    ('baoab', 1, 'S+5,0', 'loose', 'seed', 'y', 1, 'm1', True, 'heavy'),
    ('baoab', 1, 'S+5,0', 'none', 'tensor', 'all', 0, 'm3', True, 'unit'),
    ('baoab', 1, 'S+5,0', 'none', 'tensor', 'none', 1, 'big', True, 'heavy'),
    ('baoab', 2, '1,S', 'binds', 'tensor', 'none', 0, 'm0', True, 'unit'),
    ('baoab', 2, '2,3', 'binds', 'seed', 'all', 1, 'big', True, 'unit'),
    ('baoab', 2, '2,3', 'loose', 'seed', 'y', 0, 'big', True, 'heavy'),
    ('baoab', 2, '3,0', 'loose', 'tensor', 'none', 0, 'm0', True, 'unit'),
    ('baoab', 2, '3,0', 'loose', 'tensor', 'none', 0, 'm1', True, 'heavy'),
    ('baoab', 2, 'S+5,0', 'binds', 'tensor', 'all', 0, 'm2', False, 'heavy'),
    ('baoab', 2, 'S+5,0', 'none', 'seed', 'y', 1, 'm3', True, 'heavy'),
    ('baoab', 3, '1,0', 'loose', 'seed', 'y', 0, 'm0', True, 'unit'),
    ('baoab', 3, '3,0', 'binds', 'seed', 'none', 1, 'm3', False, 'heavy'),
    ('baoab', 3, 'S+5,0', 'none', 'tensor', 'all', 0, 'm1', False, 'unit'),
    ('baoab', 10, '1,0', 'binds', 'seed', 'none', 0, 'm1', True, 'heavy'),
    ('baoab', 10, '1,0', 'none', 'tensor', 'all', 1, 'm1', True, 'heavy'),
    ('baoab', 10, '1,S', 'binds', 'tensor', 'none', 1, 'm2', False, 'unit'),
    ('baoab', 10, '1,S', 'loose', 'tensor', 'all', 0, 'm3', True, 'heavy'),
    ('baoab', 10, '2,3', 'none', 'tensor', 'y', 1, 'm0', True, 'heavy'),
    ('aboba', 1, '1,0', 'binds', 'tensor', 'all', 1, 'm2', True, 'heavy'),
    ('aboba', 1, '1,S', 'binds', 'seed', 'none', 0, 'm0', True, 'heavy'),
    ('aboba', 1, '1,S', 'none', 'seed', 'all', 1, 'm2', True, 'heavy'),
    ('aboba', 1, '1,S', 'none', 'tensor', 'none', 0, 'big', False, 'heavy'),
    ('aboba', 1, '2,3', 'loose', 'seed', 'all', 0, 'm3', False, 'unit'),
    ('aboba', 1, '2,3', 'none', 'tensor', 'none', 1, 'big', False, 'unit'),
    ('aboba', 1, '3,0', 'none', 'tensor', 'all', 0, 'm2', True, 'unit'),
    ('aboba', 1, 'S+5,0', 'loose', 'seed', 'all', 0, 'big', True, 'heavy'),
    ('aboba', 1, 'S+5,0', 'none', 'seed', 'y', 1, 'm2', True, 'heavy'),
    ('aboba', 2, '1,0', 'binds', 'seed', 'y', 0, 'm1', False, 'unit'),
    ('aboba', 2, '1,0', 'none', 'tensor', 'none', 1, 'm2', True, 'unit'),
    ('aboba', 2, '1,S', 'none', 'seed', 'all', 1, 'big', False, 'unit'),
    ('aboba', 2, '1,S', 'none', 'tensor', 'y', 0, 'm3', True, 'unit'),
    ('aboba', 2, '2,3', 'none', 'seed', 'none', 1, 'm1', False, 'heavy'),
    ('aboba', 2, '3,0', 'loose', 'tensor', 'y', 1, 'big', False, 'heavy'),
    ('aboba', 2, '3,0', 'none', 'seed', 'all', 0, 'm0', False, 'heavy'),
    ('aboba', 3, '1,0', 'loose', 'tensor', 'y', 0, 'big', True, 'unit'),
    ('aboba', 3, '1,0', 'loose', 'tensor', 'y', 1, 'm0', False, 'heavy'),
    ('aboba', 3, '1,S', 'binds', 'seed', 'y', 1, 'm1', False, 'heavy'),
    ('aboba', 3, '1,S', 'loose', 'seed', 'all', 0, 'm2', True, 'unit'),
    ('aboba', 3, '1,S', 'none', 'seed', 'all', 1, 'm1', False, 'heavy'),
    ('aboba', 3, '2,3', 'binds', 'seed', 'none', 0, 'm2', True, 'unit'),
    ('aboba', 3, '2,3', 'none', 'tensor', 'all', 0, 'm3', False, 'heavy'),
    ('aboba', 3, '3,0', 'loose', 'seed', 'none', 0, 'big', False, 'heavy'),
    ('aboba', 3, '3,0', 'none', 'tensor', 'y', 1, 'm3', True, 'unit'),
    ('aboba', 3, 'S+5,0', 'binds', 'seed', 'none', 1, 'm2', True, 'heavy'),
    ('aboba', 3, 'S+5,0', 'loose', 'seed', 'none', 1, 'm1', True, 'heavy'),
    ('aboba', 10, '1,0', 'loose', 'tensor', 'none', 1, 'm3', False, 'unit'),
    ('aboba', 10, '2,3', 'binds', 'tensor', 'y', 1, 'm2', False, 'unit'),
    ('aboba', 10, '3,0', 'binds', 'tensor', 'none', 1, 'm3', False, 'unit'),
    ('aboba', 10, '3,0', 'loose', 'tensor', 'all', 1, 'm1', False, 'heavy'),
    ('aboba', 10, 'S+5,0', 'loose', 'seed', 'y', 0, 'm0', False, 'unit'),
    ('aboba', 10, 'S+5,0', 'none', 'tensor', 'y', 0, 'm0', False, 'unit'),
]
WALK_AXES = [("baoab", "aboba"), (1, 2, 3, 10), ("1,0", "3,0", "2,3", "1,S", "S+5,0"), ("none", "binds", "loose"), ("tensor", "seed"),
             ("all", "none", "y"), (0, 1), ("m0", "m1", "m2", "m3", "big"), (True, False), ("unit", "heavy")]


# ---- the update kernels, op for op in NumPy float32 (include/jamun_hip.h: jamun_baoab_pre / post, jamun_aboba_a / b) --------------------

def langevin_consts(delta, friction, M):
    """make_consts (jamun_api.cpp): computed in double from the fp32 parameters, rounded to fp32 once."""
    f = np.float32
    d, fr, u = float(f(delta)), float(f(friction)), 1.0 / float(f(M))
    return dict(u_half_delta=f(u * (d / 2)), half_delta=f(d / 2), exp_mg=f(math.exp(-fr)),
                zeta_sqrt_u=f(math.sqrt(1.0 - math.exp(-2.0 * fr)) * math.sqrt(u)))


def fma32(a, b, c):
    """fp32 fused multiply-add of arrays: the product and sum are exact in double for fp32 inputs of this size, one rounding to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def np_process_score(score, beta, clip):
    """psi = clip(score) * beta; the norm accumulates with fused multiply-adds fma(z, z, fma(y, y, x x)) (the one place, as the kernel says)."""
    f = np.float32
    p = score.astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        if clip is not None:
            norm = np.sqrt(fma32(p[:, 2], p[:, 2], fma32(p[:, 1], p[:, 1], p[:, 0] * p[:, 0])))[:, None]
            p = (p / norm) * np.minimum(norm, f(clip))
        return p * f(beta)


def np_baoab_post(v, score, k, beta, clip):
    psi = np_process_score(score, beta, clip)
    with np.errstate(invalid="ignore"):
        return v + k["half_delta"] * psi, psi


def np_baoab_pre(y, v, psi, R, k):
    vv = v + k["u_half_delta"] * psi
    yy = y + k["half_delta"] * vv
    vh = k["exp_mg"] * vv + k["zeta_sqrt_u"] * R
    return yy + k["half_delta"] * vh, vh


def np_aboba_a(y, v, k):
    return y + k["half_delta"] * v


def np_aboba_b(y, v, score, R, k, beta, clip):
    psi = np_process_score(score, beta, clip)
    with np.errstate(invalid="ignore"):
        vv = v + k["u_half_delta"] * psi
        vh = k["exp_mg"] * vv + k["zeta_sqrt_u"] * R
        vv = vh + k["half_delta"] * psi
        return y + k["half_delta"] * vv, vv
