"""Wide-path measurement on the cfg2 shape (17-atom chain x 256 walkers, sigma 0.04): ms per walk step and conformations/s (a BAOAB walk),
per-class ms per forward (``jamun_profile_*``, forwards at one fixed set of positions shared by every case) and the useful FLOP rate of the
hidden-layer conv, for

  * ``256x0e + 64x1e``, edge_attr_dim 64, and ``160x0e + 48x1e`` on the wide path (jamun_wide.hip, conv_path 3);
  * the default model forced onto the general kernels (``no_dg``, ``node_fp32``, ``edge_h_fp32``: k_conv, conv_path 0),

all in one process.  The useful rate of the hidden-layer conv is (conv0_flop_alg + conv1_flop_alg) / (conv ms per hidden layer), where conv
ms is the conv0 + conv1 profile classes of the hidden layers (the scalar- and vector-row launches) divided by their launch count / 2.

    python profiles/tools/wide_conv_profile.py [--steps 40] [--warmup 10] [--out profiles/wide_cfg2.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from jamun_amd import native, synth  # noqa: E402
from jamun_amd.data import WalkerBatch  # noqa: E402
from jamun_amd.model import Denoiser  # noqa: E402

SIGMA = 0.04


def measure(name, arch, tuning, steps, warmup):
    dev = torch.device("cuda", 0)
    native.TUNING.clear()
    native.TUNING.update(tuning)
    model = Denoiser.from_checkpoint_dict(synth.synthetic_checkpoint(arch=arch, output_gain=0.05)).to(dev)
    mols = [synth.random_chain(17, seed=0)] * 256
    batch = WalkerBatch.from_molecules(mols).to(dev)
    smp = model.sampler_for(batch, SIGMA)
    native.TUNING.clear()
    g = torch.Generator().manual_seed(0)
    y = (batch.pos.cpu() + SIGMA * torch.randn(batch.num_nodes, 3, generator=g)).to(dev)
    v = torch.randn(batch.num_nodes, 3, generator=g).to(dev)

    def walk(k):
        params = native.make_mcmc_params(k, 0.04, 1.0, 1.0, 1.0, 100.0)
        smp.walk("baoab", y, v, params, None, 1234, False, want_xhat_traj=False, want_xhat=False)

    walk(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    walk(steps)
    torch.cuda.synchronize()
    ms_step = 1e3 * (time.perf_counter() - t0) / steps
    # per-class times: forwards at the SAME positions for every case (the walks above spread differently under different models, and the
    # forming cost follows the edge count), so that the cases contract the same graph
    y_fix = (batch.pos.cpu() + SIGMA * torch.randn(batch.num_nodes, 3, generator=torch.Generator().manual_seed(1))).to(dev)
    smp.xhat(y_fix)
    smp.profile_enable(True)
    for _ in range(steps):
        smp.xhat(y_fix)
    prof = smp.profile_read()
    smp.profile_enable(False)
    st = smp.stats()
    n_hidden = model.arch["n_layers"]
    conv_ms = prof["conv0"][0] + prof["conv1"][0]
    conv_launches = prof["conv0"][1]  # one scalar-row launch per hidden layer and forward
    per_layer_ms = conv_ms / max(conv_launches, 1)
    useful = st["conv0_flop_alg"] + st["conv1_flop_alg"]
    res = dict(
        case=name,
        irreps_hidden=arch["irreps_hidden"],
        edge_attr_dim=arch["edge_attr_dim"],
        tuning=tuning,
        conv_path=st["conv_path"], init_path=st["init_path"], dg_mode=st["dg_mode"], dg_emu=st["dg_emu"],
        atoms=batch.num_nodes, walkers=batch.num_graphs, edges_of_the_profiled_forwards=st["n_edges"], steps=steps,
        ms_per_step=ms_step,
        conformations_per_s=batch.num_graphs * 1e3 / ms_step,
        per_class_ms_per_forward={k: (ms / steps, n // steps) for k, (ms, n) in prof.items() if n},
        hidden_conv_ms_per_layer=per_layer_ms,
        hidden_conv0_ms=prof["conv0"][0] / max(prof["conv0"][1], 1),
        hidden_conv1_ms=prof["conv1"][0] / max(prof["conv1"][1], 1),
        hidden_conv_useful_flop=useful,
        hidden_conv_useful_tflops=useful / (per_layer_ms * 1e-3) / 1e12,
        n_hidden_layers=n_hidden,
    )
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_cfg2.json"))
    args = ap.parse_args()
    cases = [
        ("wide_256x64", synth.default_arch(irreps_hidden="256x0e + 64x1e"), {}),
        ("wide_160x48", synth.default_arch(irreps_hidden="160x0e + 48x1e"), {}),
        ("general_default", synth.default_arch(), {"no_dg": 1, "node_fp32": 1, "edge_h_fp32": 1}),
    ]
    out = [measure(n, a, t, args.steps, args.warmup) for n, a, t in cases]
    base = out[-1]["hidden_conv_useful_tflops"]
    summary = dict(device=torch.cuda.get_device_name(0), sigma=SIGMA, cases=out,
                   wide_256x64_rate_over_general=out[0]["hidden_conv_useful_tflops"] / base)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(summary, open(args.out, "w"), indent=1)
    print("wide 256x64 useful conv rate / general k_conv rate:", summary["wide_256x64_rate_over_general"])


if __name__ == "__main__":
    main()
