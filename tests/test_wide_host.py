"""The wide path's host side (no GPU): ``jamun_model_create`` accepts Conv models of any hidden width and radial size
(``jamun_wide.hip`` serves those outside the compiled-width kernels' envelope), SeparableConv keeps its envelope, and the synthetic
checkpoints at such widths carry the parameter shapes of the reference's modules."""
import pytest
import torch

from jamun_amd import synth


def _native(arch, separable=False):
    from jamun_amd.model import Denoiser

    return Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(arch=arch, separable=separable))._native


@pytest.mark.parametrize("irreps,H", [("256x0e + 64x1e", 128), ("150x0e + 37x1e", 33), ("120x0e + 32x1e", 2), ("1x0e + 1x1e", 3)])
def test_model_create_accepts_conv_models_of_any_width_and_radial_size(irreps, H):
    nm = _native(synth.default_arch(irreps_hidden=irreps, edge_attr_dim=H))  # (raises if jamun_model_create returns an error)
    hp = nm.hparams_struct
    m0, m1 = (int(t.split("x")[0]) for t in irreps.split("+"))
    assert (hp.mul0, hp.mul1, hp.edge_attr_dim, hp.separable) == (m0, m1, H, 0)


def test_separable_conv_keeps_its_envelope_at_model_create():
    with pytest.raises(RuntimeError, match="only edge_attr_dim = 64 is supported"):
        _native(synth.default_arch(edge_attr_dim=32), separable=True)


@pytest.mark.parametrize("m0,m1,H", [(256, 64, 128), (150, 37, 33), (160, 48, 64)])
def test_synthetic_checkpoint_has_the_reference_module_shapes_at_wide_widths(m0, m1, H):
    """FullyConnectedTensorProduct(hidden x (0e + 1e) -> gate input (m0 + m1)x0e + m1x1e): paths 0x0->0, 0x1->1, 1x0->1, 1x1->0, 1x1->1
    give (m0 + m1)^2 + m0 m1 + 2 m1^2 weights per edge; the initial projector's four scalar blocks give n_emb (m0 + 2 m1).  The radial net is
    ScalarMLP(H -> [H] -> P) over [bonded (H // 2) | radial ((H + 1) // 2)] features (e3tools/nn/_conv.py:84-91, e3conv.py:42)."""
    arch = synth.default_arch(irreps_hidden=f"{m0}x0e + {m1}x1e", edge_attr_dim=H, n_layers=2)
    sd = synth.synthetic_state_dict(arch)
    P = (m0 + m1) ** 2 + m0 * m1 + 2 * m1**2
    if (m0, m1) == (256, 64):
        assert P == 126976
    n_emb = 8 + 8 + 32 + 8
    P0 = n_emb * (m0 + 2 * m1)
    for prefix, p in (("layers.0", P), ("layers.1", P), ("initial_projector", P0)):
        f = prefix + ".gated_conv.f.f.radial_nn."
        assert tuple(sd[f + "0.weight"].shape) == (H, H) and tuple(sd[f + "0.bias"].shape) == (H,)
        assert tuple(sd[f + "3.weight"].shape) == (p, H) and tuple(sd[f + "3.bias"].shape) == (p,)
    assert tuple(sd["embed_bondedness.weight"].shape) == (2, H // 2)
    # o3.Linear self-interaction (hidden -> hidden) and skip (hidden -> hidden); the head's Linear(hidden -> gate input) and Linear(-> 1x1e)
    assert sd["layers.0.gated_conv.self_interaction.weight"].numel() == m0 * m0 + m1 * m1
    assert sd["layers.0.gated_conv.skip_connection.weight"].numel() == m0 * m0 + m1 * m1
    assert sd["initial_projector.gated_conv.skip_connection.weight"].numel() == n_emb * m0
    assert sd["output_head.0.lin.weight"].numel() == m0 * (m0 + m1) + m1 * m1
    assert sd["output_head.1.weight"].numel() == m1
    assert all(torch.isfinite(v).all() for v in sd.values())
