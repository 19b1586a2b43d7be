"""Cases shared by ``test_sepconv_host.py`` (CPU) and ``test_gpu_sepconv.py`` (GPU): the molecules, checkpoints and fp64 oracle calls
that take the SeparableConv kernels (``jamun_sepconv.hip``: k_sep_fused, k_sep_linear) where no other test takes them — the second pass
of k_sep_fused's destination loop, edge slots 32..63, batches below one workgroup, channel widths inside the envelope, other noise
levels, the fused walks and ``jamun_conv_block``.  The host file asserts the premises on the CPU oracle; the GPU file holds the kernels
to the project's bounds against the same inputs."""
import functools

import torch

import _switch_cases as sc
from _switch_cases import RMSD_TOL_NM, SIGMA, rmsd  # noqa: F401  (re-exported: one set of tolerances)
from jamun_amd import synth

FEATURE_TOL = 2e-5  # per-block node features, of the block's maximum in the fp64 oracle
WAVES_PER_WORKGROUP = 8  # k_sep_fused: SF_THREADS / 64, one destination per wave
MAX_EDGE_SLOTS = 64  # sep_conv_unsupported: S > 64 is refused
RADIAL_SLOTS = 33  # JAMUN_MAX_NEIGHBORS + 1: what jamun_sampler_create reserves per destination for radial edges
TOO_MANY_SLOTS = "SeparableConv: more than 64 edge slots per destination"
NOT_A_MULTIPLE_OF_FOUR = "SeparableConv: input irreps whose per-destination sums are not a multiple of four floats"
WALK_STEPS, WALK_GAIN = 12, 0.05


# ---- molecules ----------------------------------------------------------------------------------------------------------------------

def second_pass_chains(cus):
    """Number of 33-atom chains of case 1: the first count whose atoms pass ``8 * cus`` — 63 on 256 compute units (2079 atoms)."""
    return (WAVES_PER_WORKGROUP * cus) // 33 + 1


def second_pass_molecules(cus):
    """More than ``8 * cus`` atoms, so that k_sep_fused's destination loop goes round a second time: 33-atom chains (in-degrees up to
    30) through the first pass, then forty 5-atom chains (in-degree at most 5) — the second-pass waves rewrite slot records that a
    destination of higher degree left behind.  On 256 compute units: 63 + 40 molecules, 2279 atoms, the small chains from atom 2079."""
    return ([synth.random_chain(33, seed=i) for i in range(second_pass_chains(cus))]
            + [synth.random_chain(5, seed=100 + i) for i in range(40)])


def dense_chain():
    return synth.random_chain(70, seed=3, bond=0.12, min_dist=0.13)  # (the chain of ``dense70``)


HUB, HUB_SOURCES = 35, {30: list(range(20)) + list(range(40, 50)), 31: list(range(20)) + list(range(40, 51))}


def hub_molecules(extra_bonds):
    """The dense 70-atom chain with ``extra_bonds`` (30 or 31) more bonds into atom 35, beside a 9-atom chain.  Atom 35 has one bond of
    its own, so its bonded in-degree is 31 or 32 and the edge stride 33 + 31 = 64 (the envelope's edge) or 65 (refused)."""
    m = dense_chain()
    src = torch.tensor(HUB_SOURCES[extra_bonds])
    m["bonds"] = torch.cat([m["bonds"], torch.stack([src, torch.full_like(src, HUB)])], dim=1)
    return [m, synth.random_chain(9, seed=1)]


def doubled_bond_molecules():
    """Bonds listed twice in both directions (``doubled_bonds`` of test_tail_tiles_of_the_matrix_formed_conv)."""
    mols = []
    for i, n in enumerate([33, 35, 34, 33, 40]):
        m = synth.random_chain(n, seed=70 + i)
        b = m["bonds"]
        m["bonds"] = torch.cat([b, b, b.flip(0), b.flip(0)], dim=1)
        mols.append(m)
    return mols


SMALL_BATCHES = {"atoms1": 1, "atoms2": 2, "atoms7": 7, "atoms33": 33}


@functools.lru_cache(maxsize=None)
def molecules(kind, cus=None):
    """The molecules of a case, built once per process (the tests do not modify them)."""
    if kind == "second_pass":
        return second_pass_molecules(cus)
    if kind == "dense70":
        return [dense_chain()] * 2
    if kind == "hub64":
        return hub_molecules(30)
    if kind == "hub65":
        return hub_molecules(31)
    if kind == "doubled_bonds":
        return doubled_bond_molecules()
    if kind in SMALL_BATCHES:
        return [synth.random_chain(SMALL_BATCHES[kind], seed=SMALL_BATCHES[kind])]
    if kind == "ag4":
        return [synth.ag_dipeptide()] * 4
    return sc.molecules(kind)


def bonded_in_degree(mols):
    return max(int(torch.bincount(m["bonds"][1], minlength=m["pos"].shape[0]).max()) for m in mols)


def edge_stride(mols):
    """``S`` of jamun_sampler_create: min(largest molecule - 1, 33) radial slots + the largest bonded in-degree (listings count)."""
    return max(min(max(m["pos"].shape[0] for m in mols) - 1, RADIAL_SLOTS) + bonded_in_degree(mols), 1)


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------

def _embeddings(a, b, c, d):
    return dict(atom_type_embedding_dim=a, atom_code_embedding_dim=b, residue_code_embedding_dim=c, residue_index_embedding_dim=d)


# name -> architecture overrides; (n0, n1) of the hidden layers / n0 of the initial projector in the comments
WIDTHS = {
    "h32x4": dict(irreps_hidden="32x0e + 4x1e"),  # one scalar tile (nA = 1), 4 of 32 vector lanes
    "h100x20": dict(irreps_hidden="100x0e + 20x1e"),  # masks inside the fourth scalar tile and the vector tile
    "h128x32": dict(irreps_hidden="128x0e + 32x1e"),  # the envelope: G0 = 160 = five scalar tiles, all eight waves of k_sep_linear
    "emb128": _embeddings(32, 32, 32, 32),  # initial projector with n0 = 128 (nA = 4)
    "emb20": _embeddings(4, 4, 8, 4),  # initial projector with n0 = 20
}
REFUSED_WIDTH = dict(irreps_hidden="96x0e + 18x1e")  # 4 n0 + 7 n1 = 510 floats per destination: not a multiple of four


@functools.lru_cache(maxsize=None)
def checkpoint(width=None, gain=0.5):
    over = REFUSED_WIDTH if width == "refused" else WIDTHS[width] if width else None
    return sc.checkpoint(gain=gain, separable=True, arch_over=over)


def is_separable(stats):
    return stats["conv_path"] == 0 and stats["dg_mode"] == -1  # (test_gpu_switches.py's predicate)


# ---- the fp64 oracle ----------------------------------------------------------------------------------------------------------------

def positions(topo, sigma=SIGMA, draw="fixture"):
    """Noisy positions (fp32).  ``fixture``: the draw of tests/golden/make_oracle_fixtures.py (seed 2 over the whole batch), on which
    the degree figures of the cases were taken; ``switch``: ``_switch_cases.noisy_positions``, the draw of the noise-level tests."""
    if draw == "switch":
        return sc.noisy_positions(topo, sigma)
    return topo["pos"] + sigma * torch.randn(topo["pos"].shape, generator=torch.Generator().manual_seed(2))


@functools.lru_cache(maxsize=None)
def oracle_degrees(kind, cus=None, sigma=SIGMA):
    """In-degrees of a case from the oracle's graph alone (``oracle.denoiser.xhat`` up to ``add_edges``, fp64): what the host file
    needs of the large cases without their forward."""
    from oracle import denoiser as od
    from oracle.graph import mean_center

    topo = sc.collate(molecules(kind, cus))
    y = mean_center(positions(topo, sigma).double(), topo["batch"], topo["num_graphs"])
    sig = torch.as_tensor(sigma, dtype=torch.float64)
    c_in = od.normalization_factors(sig, 0.332, 3, torch.float64)[0]
    edge_index, _ = od.add_edges(y, topo, torch.sqrt(torch.as_tensor(1.0, dtype=torch.float64) + 6 * sig**2) / c_in)
    return torch.bincount(edge_index[1], minlength=y.shape[0])


@functools.lru_cache(maxsize=None)
def forward(kind, width=None, sigma=SIGMA, cus=None, dtype=torch.float64, draw="fixture"):
    """One oracle forward of a case, computed once per process: (molecules, topology, y (fp32), x-hat, intermediates, parameters,
    hyper-parameters).  Nothing returned here is modified by the tests."""
    from oracle import denoiser as od

    mols, ck = molecules(kind, cus), checkpoint(width)
    topo, p, hp = sc.oracle_setup(mols, ck, dtype)
    y = positions(topo, sigma, draw)
    x, inter = od.xhat(y.to(dtype), topo, sigma, p, hp, return_intermediates=True)
    return mols, topo, y, x, inter, p, hp


def in_degrees(inter, n_atoms):
    return torch.bincount(inter["edge_index"][1], minlength=n_atoms)


def oracle_block(l, x_prev, topo, inter, p, hp, sigma=SIGMA):
    """Block ``l`` of the network on the edges of ``inter``, composed as ``oracle.denoiser.e3conv_forward`` composes it: l = 0 the
    initial projector on the noise-scaled embedding (``x_prev`` must be None), l >= 1  skip(x, ConvBlock_l(scale(x)))."""
    from oracle import denoiser as od
    from oracle import e3

    dtype = inter["edge_attr"].dtype
    c_noise = od.normalization_factors(torch.as_tensor(sigma, dtype=dtype), hp["average_squared_distance"], 3, dtype)[3]
    irreps_hidden, irreps_sh = e3.parse_irreps(hp["irreps_hidden"]), e3.parse_irreps(hp["irreps_sh"])
    edges = (inter["edge_index"], inter["edge_attr"], inter["edge_sh"])
    kind, sign = hp.get("conv", "conv"), hp.get("w3j_111_sign", 1.0)
    if l == 0:
        assert x_prev is None
        emb = od.atom_embedding_irreps(hp)
        x = od.noise_scaling(od.atom_embedding(topo, p, hp), c_noise, p, "initial_noise_scaling", emb)
        return od.conv_block(x, *edges, p, "initial_projector", emb, irreps_sh, irreps_hidden, kind, sign)
    xs = od.noise_scaling(x_prev, c_noise, p, f"noise_scalings.{l - 1}", irreps_hidden)
    y = od.conv_block(xs, *edges, p, f"layers.{l - 1}", irreps_hidden, irreps_sh, irreps_hidden, kind, sign)
    return od.noise_skip(x_prev, y, c_noise, p, f"skip_connections.{l - 1}", irreps_hidden)


BLOCK_KIND = "ragged"  # the batch of the jamun_conv_block tests
SCALED_BLOCKS = (1, 3, 5)
LOG2_SCALES = (-24, 24)
# what the fp32 oracle block may spend of FEATURE_TOL on the scaled inputs (a quarter; the kernel keeps three quarters), and what it
# does spend: the largest deviation from the fp64 oracle block over blocks 1, 3, 5 of ``ragged``, of the block maximum, measured on the
# CPU (test_sepconv_host.py asserts that the oracle stays within twice these — its summation order moves with the thread count)
REF_SHARE = FEATURE_TOL / 4
SCALED_REF_DEV = {-24: 7.3e-8, 24: 3.4e-7}


def scaled_block_case(l, log2_scale, dtype=torch.float64):
    """(input, oracle output) of block ``l`` on the fp64 oracle's own features of ``ragged`` times 2^log2_scale, the block evaluated in
    ``dtype`` on that input rounded to fp32 first (what the kernel is fed)."""
    _, topo, _, _, inter, p, hp = forward(BLOCK_KIND, dtype=dtype)
    x_in = (forward(BLOCK_KIND)[4][f"x{l - 1}"] * 2.0**log2_scale).float()
    return x_in, oracle_block(l, x_in.to(dtype), topo, inter, p, hp)


def block_error(a, ref):
    """Largest deviation of a block's features from the reference, of the reference's maximum (the project's per-block measure)."""
    return (a.double().cpu() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-6)


# ---- walks --------------------------------------------------------------------------------------------------------------------------

def walk_inputs(kind="ag4", steps=WALK_STEPS, seed=42):
    """Recorded noise of a walk as test_wide_baoab_walk_matches_the_oracle_walk draws it: row 0 -> y0, row 1 -> v0, the rest per step."""
    topo = sc.collate(molecules(kind))
    noise = torch.randn(steps + 1, topo["pos"].shape[0], 3, generator=torch.Generator().manual_seed(seed))
    return topo, noise, topo["pos"] + SIGMA * noise[0]


WALK_MCMC = dict(delta=0.04, friction=1.0, M=1.0, inverse_temperature=1.0, score_fn_clip=100.0)


@functools.lru_cache(maxsize=None)
def oracle_walk(integrator, kind="ag4", steps=WALK_STEPS):
    """``oracle.walk.walk_jump`` in fp64 on the contractive separable checkpoint (gain 0.05), trajectory saved."""
    from oracle import denoiser as od
    from oracle import walk as ow

    mols = molecules(kind)
    topo, p, hp = sc.oracle_setup(mols, checkpoint(gain=WALK_GAIN), torch.float64)
    _, noise, y0 = walk_inputs(kind, steps)
    return ow.walk_jump(lambda t: od.score(t, topo, SIGMA, p, hp), lambda t: od.xhat(t, topo, SIGMA, p, hp), getattr(ow, integrator),
                        y0.double(), noise[1].double(), ow.RecordedNoise(noise[2:]), steps=steps, save_trajectory=True, **WALK_MCMC)
