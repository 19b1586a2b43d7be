"""CPU-side premises of ``test_gpu_sepconv.py`` (no GPU): what the cases of ``_sepconv_cases.py`` are on the oracle alone, so that the
GPU tests cannot pass without entering the paths they name.

* the in-degrees of the second-pass batch and of the edge-slot cases, and the edge stride ``S`` on both sides of the 64-slot envelope;
* the oracle block composed in ``_sepconv_cases.oracle_block`` against the oracle's own forward, layer by layer, exactly;
* the oracle runs every accepted width, and the widths do what their names say (masks inside a tile, whole tiles, one tile);
* the reference's own share of the bounds: the fp32 oracle against the fp64 oracle over the noise levels and on block inputs scaled
  by 2^-24 / 2^24.
"""
import pytest
import torch

import _sepconv_cases as sp
import _switch_cases as sc

CUS = 256  # compute units of the part the figures below were taken for (the GPU test reads the count from the device)


def test_second_pass_batch_premises():
    """Case 1 on 256 compute units: 63 + 40 molecules, 2279 atoms > 8 * 256, so k_sep_fused's grid (min(CUs, ceil(n / 8)) workgroups of
    eight waves) covers atoms 0..2047 in its first pass and the rest in a second.  First-pass destinations have in-degrees up to 30
    (mean 15.0); every atom from 2079 on — 200 of the 231 second-pass destinations — has at most 5, so most second-pass waves rewrite
    records below a longer list left in LDS, and the 31 atoms before them (in-degrees up to 29) keep the pass from being all short."""
    mols = sp.molecules("second_pass", CUS)
    n = sum(m["pos"].shape[0] for m in mols)
    assert (sp.second_pass_chains(CUS), len(mols), n) == (63, 103, 2279) and n > 2048
    assert (n + 7) // 8 > CUS  # the grid is clamped to the compute units: the loop goes round again
    deg = sp.oracle_degrees("second_pass", CUS)
    first, second = deg[: 8 * CUS], deg[8 * CUS :]
    assert int(first.max()) == 30 and abs(first.float().mean().item() - 15.0) < 0.1
    assert int(deg[2079:].max()) == 5 and int(second[:31].max()) == 29
    # a second-pass destination d is served by the wave that served d - 8 * CUS: most inherit a longer list
    assert (second < first[: second.numel()]).float().mean().item() > 0.8
    for cus in (64, 104, 304):  # other parts: the 33-atom chains alone pass 8 * CUs, by less than one chain
        assert 0 < 33 * sp.second_pass_chains(cus) - 8 * cus <= 33


def test_edge_slot_premises():
    """Case 2.  ``dense70`` x 2: in-degrees 32, 33 and 34 on 5, 69 and 14 atoms (the second M tile of k_sep_fused holds one or two
    rows).  The hub: 30 more bonds into atom 35 give a bonded in-degree of 31, S = 33 + 31 = 64, 63 in-edges at the hub (32 radial,
    the cap, + 31 bonded) and 41 atoms above 32; one bond more gives 32 and S = 65.  Doubled bonds: bonded in-degree 6, S = 39."""
    deg = sp.oracle_degrees("dense70")
    assert [int((deg == v).sum()) for v in (32, 33, 34)] == [5, 69, 14] and int(deg.max()) == 34
    assert sp.edge_stride(sp.molecules("dense70")) == 34
    hub = sp.molecules("hub64")
    assert sp.bonded_in_degree(hub) == 31 and sp.edge_stride(hub) == 64 == sp.MAX_EDGE_SLOTS
    deg = sp.oracle_degrees("hub64")
    assert int(deg[sp.HUB]) == 63 == int(deg.max()) and int((deg > 32).sum()) == 41
    over = sp.molecules("hub65")
    assert sp.bonded_in_degree(over) == 32 and sp.edge_stride(over) == 65
    assert over[0]["bonds"].shape[1] == hub[0]["bonds"].shape[1] + 1
    dbl = sp.molecules("doubled_bonds")
    assert sp.bonded_in_degree(dbl) == 6 and sp.edge_stride(dbl) == 39 and int(sp.oracle_degrees("doubled_bonds").max()) >= 30


def test_small_batch_premises():
    """Case 3: 1, 2, 7 and 33 atoms, each a batch on its own.  The single atom has no edge (its x-hat is finite in the oracle: the
    mean over no messages is 0); 33 atoms are one full tile of k_sep_linear and a second with one row."""
    for kind, n in sp.SMALL_BATCHES.items():
        mols, _, y, x, inter, _, _ = sp.forward(kind)
        assert len(mols) == 1 and y.shape[0] == n and torch.isfinite(x).all()
        assert sp.edge_stride(mols) == max(n, 1)  # n - 1 radial slots + one bond, and never below one slot
    deg1 = sp.in_degrees(sp.forward("atoms1")[4], 1)
    assert deg1.tolist() == [0] and sp.forward("atoms1")[4]["edge_index"].shape[1] == 0
    assert 33 % 32 == 1


@pytest.mark.parametrize("width", list(sp.WIDTHS))
def test_oracle_runs_every_accepted_width(width):
    """Case 4: the oracle builds and runs each width; the channel counts are the ones the kernel masks are meant to meet."""
    from jamun_amd.synth import _irreps_muls

    _, _, y, x, inter, p, hp = sp.forward("ragged", width=width)
    assert torch.isfinite(x).all() and hp["conv"] == "separable"
    m0, m1 = _irreps_muls(hp["irreps_hidden"])
    n_emb = 2 * hp["atom_type_embedding_dim"] + hp["residue_code_embedding_dim"] + hp["residue_index_embedding_dim"]
    assert inter["x0"].shape[1] == m0 + 3 * m1
    assert p["layers.0.gated_conv.f.f.radial_nn.3.weight"].shape[0] == 2 * m0 + 3 * m1  # depth-wise weights per edge
    assert p["initial_projector.gated_conv.f.f.radial_nn.3.weight"].shape[0] == 2 * n_emb
    want = {"h32x4": (32, 4, 56), "h100x20": (100, 20, 56), "h128x32": (128, 32, 56), "emb128": (120, 32, 128), "emb20": (120, 32, 20)}
    assert (m0, m1, n_emb) == want[width]
    assert m0 <= 128 and m1 <= 32 and m1 % 4 == 0 and n_emb <= 128 and m0 + m1 <= 160  # inside the envelope of sep_conv_unsupported
    assert (4 * m0 + 7 * m1) % 4 == 0 and (4 * n_emb) % 4 == 0  # per-destination sums: K0 + 3 K1 floats


def test_refused_width_premise():
    """96x0e + 18x1e: inside the widths of the envelope, but 4 n0 + 7 n1 = 510 floats per destination is no multiple of four."""
    from jamun_amd.synth import _irreps_muls

    m0, m1 = _irreps_muls(sp.REFUSED_WIDTH["irreps_hidden"])
    assert m0 <= 128 and m1 <= 32 and m0 + m1 <= 160 and m1 % 4 != 0 and (4 * m0 + 7 * m1) % 4 != 0


def test_composed_oracle_block_reproduces_the_forward_exactly():
    """``oracle_block`` applied to the forward's own x_{l-1} gives the forward's x_l bit for bit, for every block."""
    _, topo, _, _, inter, p, hp = sp.forward(sp.BLOCK_KIND)
    x = None
    for l in range(hp["n_layers"] + 1):
        x = sp.oracle_block(l, x, topo, inter, p, hp)
        assert torch.equal(x, inter[f"x{l}"]), l


def test_fp32_oracle_block_on_scaled_inputs():
    """Case 7's share of the reference: the fp32 oracle block against the fp64 oracle block on the same input (the fp64 features of
    ``ragged`` times 2^-24 / 2^24, rounded to fp32), largest deviation of the block maximum over blocks 1, 3, 5.  Measured 7.3e-8 at
    2^-24 and 3.4e-7 at 2^24: well inside a quarter of the 2e-5 bound (5e-6), so the GPU test keeps 2^+-24 and the bound as it is."""
    for s in sp.LOG2_SCALES:
        worst = 0.0
        for l in sp.SCALED_BLOCKS:
            x_in, r64 = sp.scaled_block_case(l, s)
            x_in32, r32 = sp.scaled_block_case(l, s, torch.float32)
            assert torch.equal(x_in, x_in32) and torch.isfinite(r32).all()
            assert 2.0 ** (s - 3) < x_in.abs().max().item() < 2.0 ** (s + 8)  # the input really is that small / large
            worst = max(worst, sp.block_error(r32, r64))
        print(f"fp32 oracle block against fp64 at 2^{s}: {worst:.3e} of the block maximum")
        assert worst <= 2 * sp.SCALED_REF_DEV[s] and worst <= sp.REF_SHARE, (s, worst)


def test_fp32_oracle_against_fp64_over_the_noise_levels_on_the_separable_checkpoint():
    """Case 5's share of the reference: measured 4.0e-8 / 3.3e-8 / 4.7e-8 / 3.5e-8 nm RMSD at sigma 0.01 / 0.1 / 0.4 / 1.0 — within a
    quarter of the tolerance, so the bound of ``_switch_cases.xhat_bound`` (1e-5 nm at every level) holds for this checkpoint too; the
    two precisions build the same edges, and neighbouring levels differ by more than 100 tolerances."""
    prev = None
    for sigma in sc.SIGMAS:
        _, topo, y, x64, i64, p, hp = sp.forward("ragged", sigma=sigma, draw="switch")
        _, _, _, x32, i32, _, _ = sp.forward("ragged", sigma=sigma, dtype=torch.float32, draw="switch")
        dev = sc.rmsd(x32, x64)
        print(f"separable ragged sigma {sigma}: fp32 oracle against fp64 {dev:.3e} nm")
        assert dev <= sc.REF_SHARE_NM and sc.xhat_bound("ragged", sigma) == sc.RMSD_TOL_NM
        assert torch.equal(i32["edge_index"], i64["edge_index"])
        if prev is not None:
            from oracle import denoiser as od

            assert sc.rmsd(x64, od.xhat(y.double(), topo, prev, p, hp)) >= sc.DID_SOMETHING
        prev = sigma


def test_walk_premises():
    """Case 6: the fp64 oracle walks save one x-hat frame per step, and the two integrators part by more than 100 tolerances."""
    b, a = sp.oracle_walk("baoab"), sp.oracle_walk("aboba")
    assert b["xhat_traj"].shape == a["xhat_traj"].shape == (sp.WALK_STEPS, 40, 3) and b["xhat_traj"].dtype == torch.float64
    assert sc.rmsd(b["xhat_traj"][-1], a["xhat_traj"][-1]) >= sc.DID_SOMETHING
