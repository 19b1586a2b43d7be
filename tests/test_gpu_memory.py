"""GPU tests of the sampler's device-memory ownership (``-m gpu``): every buffer of a ``jamun_sampler`` comes from its ``DevArena``
(``jamun_host.h``), so destroying a sampler, and a create that fails half-way, give back exactly what was allocated.  The figures are the
library's own counters (``jamun_debug_live_allocations``: allocations and requested bytes of this process), read after a device
synchronisation and compared for equality — other users of the card cannot move them."""
import functools
import gc
import re

import pytest
import torch

import _select_cases as sel
import _sepconv_cases as sp
from jamun_amd import native, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SIGMA = sp.SIGMA
WIDE_ARCH = sel.WIDE_ARCH_H160  # ``h160x48`` of test_gpu_wide.py
SKIP_KEY = "g.skip_connections.0.weights.scale_predictor.0.weight"  # read between build_layer and the layer's place in the sampler
RADIAL_KEY = "g.layers.0.gated_conv.f.f.radial_nn.3.weight"  # read inside build_layer, after the node-update weights were uploaded


def _live():
    gc.collect()
    torch.cuda.synchronize()
    return native.live_allocations()


@functools.lru_cache(maxsize=None)
def _model(kind, without=None):
    from jamun_amd.model import Denoiser

    ck = {"conv": lambda: synth.synthetic_checkpoint(output_gain=0.5), "separable": sp.checkpoint,
          "wide": lambda: synth.synthetic_checkpoint(arch=synth.default_arch(**WIDE_ARCH), output_gain=0.5)}[kind]()
    if without:
        assert without in ck["state_dict"]
        ck = dict(ck, state_dict={k: v for k, v in ck["state_dict"].items() if k != without})
    return Denoiser.from_checkpoint_dict(ck).to(DEV)


@functools.lru_cache(maxsize=None)
def _batch(mols_kind):
    from jamun_amd.data import WalkerBatch

    mols = sel.molecules(mols_kind)
    return WalkerBatch.from_molecules(list(mols)).to(DEV)


def _create(kind, mols_kind="ag4", tuning=None, without=None):
    return native.NativeSampler(_model(kind, without)._native, SIGMA, _batch(mols_kind), DEV, tuning=tuning)


def _y(mols_kind="ag4"):
    pos = _batch(mols_kind).pos
    return pos + SIGMA * torch.randn(pos.shape, generator=torch.Generator().manual_seed(5)).to(DEV)


ROUND_TRIPS = sel.ROUND_TRIPS  # name -> (model, molecules, tuning, what the stats must say so that the case is the path it names)


@pytest.mark.parametrize("name", list(ROUND_TRIPS))
def test_create_then_destroy_returns_every_allocation(name):
    kind, mols_kind, tuning, is_the_path = ROUND_TRIPS[name]
    _model(kind), _batch(mols_kind)
    count0, bytes0 = _live()
    smp = _create(kind, mols_kind, tuning)
    assert is_the_path(smp.stats()), smp.stats()
    count1, bytes1 = _live()
    print(f"{name}: {count1 - count0} allocations, {bytes1 - bytes0} bytes while the sampler lives")
    assert count1 > count0 and bytes1 > bytes0 and bytes1 > 0
    del smp
    assert _live() == (count0, bytes0)


def test_no_dg_sampler_holds_less_than_the_default_one():
    """The tile plan's weights (``LayerDev::dg``) are released at create when the plan is not selected, not at destroy."""
    count0, bytes0 = _live()
    held = {}
    for name, tuning in (("default", None), ("no_dg", {"no_dg": 1})):
        smp = _create("conv", "ag4", tuning)
        held[name] = _live()[1] - bytes0
        del smp
        assert _live() == (count0, bytes0)
    print(f"bytes held on ag4: {held}")
    assert 0 < held["no_dg"] < held["default"]


FAILURES = {  # name -> (model, model without this tensor, molecules, tuning, the parent's error text)
    "a_missing_skip_mix": ("conv", SKIP_KEY, "ag4", None, re.escape("missing checkpoint tensor: " + SKIP_KEY[2:])),
    "b_missing_radial_weight": ("conv", RADIAL_KEY, "ag4", None, re.escape("missing checkpoint tensor: " + RADIAL_KEY[2:])),
    "c_stride_65_refused": ("separable", None, "hub65", None, re.escape(sp.TOO_MANY_SLOTS)),
    "d_selfcheck_2": ("conv", None, "ag4", {"selfcheck": 2}, "self-check failed.*must not sample"),
    "e_selfcheck_7": ("conv", None, "ag4", {"selfcheck": 7}, re.escape("jamun_tuning.selfcheck must be -1 (off), 0 (default: on), 1 (on) or 2 (on, with an injected fault)")),
}


@pytest.mark.parametrize("name", list(FAILURES))
def test_failed_create_returns_every_allocation_and_the_next_sampler_is_the_same(name):
    kind, without, mols_kind, tuning, message = FAILURES[name]
    _model(kind, without), _batch(mols_kind)
    y = _y()
    before = _create(kind)
    if name == "d_selfcheck_2":
        assert before.stats()["conv_path"] == 2  # (the self-check runs on the tile plan only)
    x_before = before.xhat(y)
    del before
    count0, bytes0 = _live()
    for _ in range(5):
        with pytest.raises(RuntimeError, match=message):
            _create(kind, mols_kind, tuning, without)
        assert _live() == (count0, bytes0)
        after = _create(kind)
        assert torch.equal(after.xhat(y), x_before)
        del after
        assert _live() == (count0, bytes0)
