"""Kernel-selection expectations shared by the GPU tests that read ``jamun_sampler_stats`` (``test_gpu_switches.py``, ``test_gpu_memory.py``,
``test_gpu_variants.py``) and by ``test_select_host.py``, which asks the same questions of ``select_kernels`` on the CPU
(``jamun_debug_select_kernels``): one list of (batch, switches, what the stats must say), read by both sides.  Also the inputs of the
selection golden ``tests/golden/select_kernels.json`` and the host-side restatement of what packing produces for the default widths."""
import importlib.util
import os

import numpy as np

import _sepconv_cases as sp
import _switch_cases as sc
from jamun_amd import synth

CUS = 256  # compute units of an MI355X


# ---- what jamun_sampler_stats must report (predicates on its dict) ---------------------------------------------------------------------

def default_kernels(st):
    return st["conv_path"] == 2 and st["dg_mode"] in (4, 5) and st["dg_emu"] == 1


def is_wide(st):
    return (st["conv_path"], st["init_path"], st["dg_mode"], st["dg_emu"]) == (3, 6, -1, 0)


# (name, jamun_tuning, predicate) for a Conv checkpoint of the default widths; for SeparableConv; for the wide path
CONV_SELECTIONS = [
    ("default", None, default_kernels),
    ("no_dg", {"no_dg": 1}, lambda st: st["conv_path"] == 0 and st["init_path"] == 0),
    ("no_mf", {"no_mf": 1}, lambda st: st["conv_path"] == 2 and st["dg_mode"] != 4),
]
SEPARABLE_SELECTIONS = [("separable", None, sp.is_separable)]
WIDE_SELECTIONS = [("wide", None, is_wide)]
WIDE_ARCH_H32 = dict(edge_attr_dim=32)  # test_gpu_wide.py's H32 preset: a radial size outside the compiled kernels' envelope
WIDE_ARCH_H160 = dict(irreps_hidden="160x0e + 48x1e")  # ``h160x48`` of test_gpu_wide.py

# (molecules, architecture, [(name, tuning, predicate)]): each conv kernel family on the batch that selects it
FAMILY_CASES = [
    ("chain17x6", "conv", [
        ("k_conv_mf + k_conv_mfi", None, lambda st: st["dg_mode"] == 4 and st["init_path"] == 3 and st["n_tail_tiles"] == 0),
        ("k_conv_dg + k_conv_init_v", {"no_mf": 1, "no_mfi": 1}, lambda st: st["conv_path"] == 2 and st["dg_mode"] in (0, 1, 2, 3) and st["init_path"] == 2),
        ("k_conv", {"no_dg": 1}, lambda st: st["conv_path"] == 0 and st["init_path"] == 0)]),
    ("ragged", "conv", [("k_conv_mf + k_conv_mfx", None, lambda st: st["dg_mode"] == 4 and st["init_path"] == 4)]),
    ("chain33x4", "conv", [("k_tail_form / k_tail_contract", None, lambda st: st["dg_mode"] == 4 and st["n_tail_tiles"] >= 4)]),
    ("chig93x2", "conv", [("k_conv_ml + k_conv_mlx", None, lambda st: st["dg_mode"] == 5 and st["init_path"] == 5)]),
    ("chain17x6", "separable", SEPARABLE_SELECTIONS),
    ("chain17x6", "wide", WIDE_SELECTIONS),
]

# name -> (model, molecules, tuning, predicate): the samplers test_gpu_memory.py creates and destroys
ROUND_TRIPS = {
    "default": ("conv", "ag4", None, lambda st: st["conv_path"] == 2),
    "no_dg": ("conv", "ag4", {"no_dg": 1}, lambda st: st["conv_path"] == 0 and st["dg_mode"] == -1),
    "separable": ("separable", "ag4", None, sp.is_separable),
    "wide": ("wide", "ag4", None, lambda st: st["conv_path"] == 3),  # (h160x48)
    "selfcheck_off": ("conv", "ag4", {"selfcheck": -1}, lambda st: st["conv_path"] == 2),
    "mode5": ("conv", "chain70x2", None, lambda st: st["dg_mode"] == 5),
    "tail_tiles": ("conv", "doubled_bonds", None, lambda st: st["dg_mode"] == 4 and st["n_tail_tiles"] > 0),
}

# (molecules) -> exact stats fields of the default-width Conv model (test_gpu_variants.py: the presets ``nl2``, ``trained`` and the default
# point change weights and depth, not widths)
VARIANT_STATS = {
    ("nl2", "ragged"): dict(dg_mode=4, dg_emu=1),
    ("trained", "chain17x6"): dict(dg_mode=4, init_path=3, dg_emu=1),
    ("trained", "ragged"): dict(dg_mode=4, init_path=4, dg_emu=1),
    ("trained", "chig93x2"): dict(dg_mode=5, init_path=5, dg_emu=1, ml_window=96),  # the reference's chignolin shape (93 heavy atoms) on k_conv_ml / k_conv_mlx
    ("default", "dipep48"): dict(dg_mode=4, dg_emu=1, init_path=4),
}


def anchors():
    """Every expectation above as (id, molecules, architecture, tuning, predicate) for the host test."""
    out = []
    for kind in ("chain17x6", "ragged", "chig93x2"):  # test_forward_without_centring_on_translated_walkers
        for arch, sel in (("conv", CONV_SELECTIONS), ("separable", SEPARABLE_SELECTIONS), ("wide", WIDE_SELECTIONS)):
            out += [(f"switches-{kind}-{name}", kind, arch, tuning, ok) for name, tuning, ok in sel]
    for kind, arch, sel in FAMILY_CASES:
        out += [(f"family-{kind}-{name}", kind, arch, tuning, ok) for name, tuning, ok in sel]
    out += [(f"memory-{name}", kind, "wide160" if arch == "wide" else arch, tuning, ok) for name, (arch, kind, tuning, ok) in ROUND_TRIPS.items()]
    for (variant, kind), want in VARIANT_STATS.items():
        out.append((f"variants-{variant}-{kind}", kind, "nl2" if variant == "nl2" else "conv", None,
                    lambda st, want=want: all(st[k] == v for k, v in want.items())))
    return out


# ---- the batches and models of those cases, on the CPU ---------------------------------------------------------------------------------

def molecules(kind):
    if kind == "chain70x2":
        return [synth.random_chain(70, seed=0)] * 2
    if kind == "dipep48":
        spec = importlib.util.spec_from_file_location("make_oracle_fixtures", os.path.join(os.path.dirname(__file__), "golden", "make_oracle_fixtures.py"))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        return mk.molecules(kind)
    return list(sp.molecules(kind))


ARCH_OVER = {"conv": {}, "nl2": dict(n_layers=2), "separable": {}, "wide": WIDE_ARCH_H32, "wide160": WIDE_ARCH_H160}


def hparams(arch):
    """The jamun_hparams fields kernel selection reads, of a test architecture."""
    from jamun_amd.native import parse_hidden_irreps

    a = synth.default_arch(**ARCH_OVER[arch])
    m0, m1 = parse_hidden_irreps(a["irreps_hidden"])
    return dict(n_layers=a["n_layers"], mul0=m0, mul1=m1, edge_attr_dim=a["edge_attr_dim"], separable=int(arch == "separable"),
                emb_dim=[a["atom_type_embedding_dim"], a["atom_code_embedding_dim"], a["residue_code_embedding_dim"], a["residue_index_embedding_dim"]])


def default_layouts(n_layers, n_uniq, no_dg=False):
    """What jamun_pack.cpp produces for a Conv model of the default widths (120x0e + 32x1e, 56 embedding channels): every hidden layer
    with the weights of k_conv_dg, of the matrix-formed kernels and of the tail tiles unless ``no_dg``; the initial projector with the
    table of k_conv_init_v, the table of k_conv_mfi up to 128 distinct rows (1, 2 or 4 selector tiles of 32 rows), the weights of
    k_conv_mfx and five scalar output tiles.  -> (hidden, layer0, have_atom_uid)"""
    hidden = [(not no_dg,) * 3] * n_layers
    tabw = n_uniq <= 128
    return hidden, (1, int(tabw), (1 if n_uniq <= 32 else 2 if n_uniq <= 64 else 4) if tabw else 0, 1, 5), True


NO_LAYOUTS = ((0, 0, 0, 0, 5), False)  # SeparableConv and the wide path pack none of these layouts


def select(mols, arch, tuning):
    """The host selection for molecules of a test batch and a test architecture -> the dict of native.select_kernels with every list."""
    from jamun_amd import native
    from jamun_amd.data import WalkerBatch

    b = WalkerBatch.from_molecules(mols)
    hp = hparams(arch)
    n_uniq = sc.embedding_rows(mols, False)
    if arch in ("conv", "nl2"):
        hidden, layer0, uid = default_layouts(hp["n_layers"], n_uniq, bool((tuning or {}).get("no_dg")))
    else:
        hidden, (layer0, uid) = [(0, 0, 0)] * hp["n_layers"], NO_LAYOUTS
    return native.select_kernels(hp, tuning, b.ptr.numpy(), b.bonds.numpy(), CUS, n_uniq, uid, hidden, layer0, lists=native.SELECT_LISTS)


def as_stats(sel):
    """The plan as jamun_sampler_stats reports it: SeparableConv in the general kernels' slot, the tile plan's fields only with CONV_DG."""
    dg = sel["conv_path"] == 2
    return dict(conv_path=max(0, sel["conv_path"]), init_path=max(0, sel["init_path"]), dg_mode=sel["dg_mode"] if dg else -1,
                dg_emu=0 if sel["conv_path"] == 3 else sel["dg_emu"] if dg else -1, dg_row_blocks=int(dg and sel["row_blocks"]),
                n_tail_tiles=sel["n_tail_tiles"], n_tail=sel["n_tail"], mf_nks=sel["mf_nks"] if dg and sel["dg_mode"] == 4 else 0,
                ml_window=sel["ml_window"] if dg and sel["dg_mode"] == 5 else 0, n_slices=sel["n_slabs"] if dg else 8, edge_stride=sel["S"])


# ---- the golden: synthetic chains, inputs as parameters --------------------------------------------------------------------------------

def chain_topology(sizes, listings=1):
    """ptr and bonds of chains of the given sizes: atom i bonded to i + 1, each bond listed ``listings`` times in both directions."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    src = np.concatenate([np.arange(ptr[g], ptr[g + 1] - 1) for g in range(len(sizes))] + [np.zeros(0, np.int64)]).astype(np.int64)
    one = np.stack([np.concatenate([src, src + 1]), np.concatenate([src + 1, src])])
    return ptr, np.concatenate([one] * listings, axis=1)


def _g(sizes, tuning=None, arch="conv", n_uniq=16, cus=CUS, listings=1, layouts=None):
    return dict(sizes=list(sizes), tuning=dict(tuning or {}), arch=arch, n_uniq=n_uniq, cus=cus, listings=listings, layouts=layouts)


def golden_inputs():
    """The deterministic case list of tests/golden/select_kernels.json (tests/golden/make_select_kernels.py records it)."""
    no_mf = {"no_mf": 1}
    cases = [
        _g([17] * 64), _g([17] * 64, n_uniq=105), _g([17] * 64, n_uniq=200), _g([33] * 64), _g([33] * 64, {"no_tail": 1}), _g([33] * 64, {"no_mfi": 1}),
        _g([33] * 64, {"no_short_k": 1}), _g([20, 20] * 8), _g([57] * 32, n_uniq=60), _g([70] * 16), _g([93] * 8), _g([120] * 4), _g([166] * 4),
        _g([166] * 4, {"no_mfi": 1}), _g([93] * 2, {"no_mfi": 1}), _g([200] * 2), _g([5, 17, 33, 9, 57, 2, 1, 29], n_uniq=105),
        _g([63, 9, 101, 64, 120, 3, 77], n_uniq=40), _g([1]), _g([2, 1, 1]), _g([33, 35, 34, 33, 40], listings=2), _g([17] * 6, listings=3),
        _g([17] * 64, no_mf), _g([33] * 64, no_mf), _g([100] * 8, no_mf), _g([250] * 2, no_mf), _g([250] * 2, {"no_mf": 1, "dg_no_alt": 1}),
        _g([17] * 64, {"no_mf": 1, "dg_no_sp": 1}), _g([17] * 64, {"no_mf": 1, "dg_no_sp": 1, "dg_no_sph": 1}), _g([17] * 64, {"dg_fp32": 1}),
        _g([93] * 8, {"no_ml": 1}), _g([17] * 64, {"no_mfi": 1}), _g([17] * 64, {"no_mfi": 1, "no_init_v": 1}), _g([17] * 64, {"no_dg": 1}),
        _g([17] * 64, {"dg_kgroups": 4}), _g([93] * 8, {"dg_kgroups": 8}), _g([33] * 64, {"dg_kgroups": 2, "seg_cost_tenths": 50}),
        _g([17] * 64, {"seg_cost_tenths": -1}), _g([17] * 64, cus=80), _g([33] * 16, cus=8), _g([93] * 8, cus=250, tuning={"dg_kgroups": 4}),
        _g([17] * 64, arch="separable"), _g([17] * 64, arch="wide"), _g([17] * 64, arch="wide160"), _g([17] * 64, arch="nl2"),
        # layouts packing can leave out: no table of k_conv_mfi, no k_conv_mfx weights, no tail weights, no matrix-formed weights, no table at all
        _g([17] * 64, layouts=dict(hidden=(1, 1, 1), layer0=(1, 0, 0, 1, 5))), _g([17] * 64, layouts=dict(hidden=(1, 1, 1), layer0=(1, 0, 0, 0, 5))),
        _g([33] * 64, layouts=dict(hidden=(1, 1, 0), layer0=(1, 1, 1, 1, 5))), _g([17] * 64, layouts=dict(hidden=(1, 0, 0), layer0=(1, 1, 1, 1, 5))),
        _g([33] * 64, layouts=dict(hidden=(1, 1, 1), layer0=(0, 0, 0, 0, 5))), _g([17] * 64, layouts=dict(hidden=(1, 1, 1), layer0=(1, 1, 1, 1, 4))),
    ]
    return cases


def golden_select(case):
    from jamun_amd import native

    hp = hparams(case["arch"])
    ptr, bonds = chain_topology(case["sizes"], case["listings"])
    if case["layouts"]:
        hidden, layer0, uid = [tuple(case["layouts"]["hidden"])] * hp["n_layers"], tuple(case["layouts"]["layer0"]), bool(case["layouts"]["layer0"][0] or case["layouts"]["layer0"][1])
    elif case["arch"] in ("conv", "nl2"):
        hidden, layer0, uid = default_layouts(hp["n_layers"], case["n_uniq"], bool(case["tuning"].get("no_dg")))
    else:
        hidden, (layer0, uid) = [(0, 0, 0)] * hp["n_layers"], NO_LAYOUTS
    return native.select_kernels(hp, case["tuning"], ptr, bonds, case["cus"], case["n_uniq"], uid, hidden, layer0, lists=native.SELECT_LISTS)
