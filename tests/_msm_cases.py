"""What test_msm_host.py and test_gpu_msm.py share: independent double loops for the four reductions, frames on which a fused multiply-add
would choose another centre than the specification, exact ties, a block-structured transition matrix, and the dipeptide whose psi hops
between three wells (the fixture of the meter) with the measured stability of its outputs.

FMA-SENSITIVE FRAMES.  `FMA_CASES[d]` holds frames ``y`` nearly equidistant from two centres ``c0``, ``c1`` (found by a random search on
the CPU: ``y`` = the midpoint plus a vector orthogonal to ``c1 - c0``, so that the two squared distances agree to the last bits), frozen
as hexadecimal floats, each with the label of the specification (a subtraction, a multiplication and an addition, each rounded) and the
label of the CONTRACTED evaluation ``acc = fl(acc + diff * diff)`` (`fused_distance`: exact rational arithmetic, rounded once per step).
The two labels differ on every frozen frame: a kernel that lets the compiler contract fails on them.

THE METER FIXTURE.  psi of ALA hops between the wells `WELLS` as a Markov chain that leaves its well with probability 1 / `DWELL` per
frame (to either other well alike), with `NOISE` rad of noise on psi and on phi of GLY.  The wells are 2 rad apart and the noise 0.1 rad,
so the microstates of k-means lie inside the wells and no frame sits within 1e-9 of a boundary between two centres: moving every projected
value by `_tica_cases.METER_TOLERANCE["tic01"]` changes no label (test_msm_host.py holds the fixture to that), and with the labels every
integer output and every float derived from integers stays as it is.
"""
import functools
from fractions import Fraction

import numpy as np
import torch

import _tica_cases as tc


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


# ---- independent double loops ------------------------------------------------------------------------------------------------------------------------

def spec_distance(y, c) -> float:
    """The specification's squared distance of one row to one centre in plain Python floats: three roundings per column."""
    acc = 0.0
    for j in range(len(y)):
        diff = float(y[j]) - float(c[j])
        sq = diff * diff
        acc = acc + sq
    return acc


def fused_distance(y, c) -> float:
    """The contracted evaluation: ``diff`` rounded, then ``acc + diff * diff`` formed exactly and rounded once (a fused multiply-add)."""
    acc = 0.0
    for j in range(len(y)):
        diff = float(y[j]) - float(c[j])
        acc = float(Fraction(acc) + Fraction(diff) * Fraction(diff))  # (Fraction -> float rounds to nearest)
    return acc


def assign_loop(y, centers, distance=spec_distance):
    labels, sq = [], []
    for row in y:
        if not all(np.isfinite(v) for v in row):
            labels.append(-1)
            sq.append(float("nan"))
            continue
        best, best_c = None, -1
        for c in range(len(centers)):
            acc = distance(row, centers[c])
            if best is None or acc < best:
                best, best_c = acc, c
        labels.append(best_c)
        sq.append(best)
    return np.array(labels, dtype=np.int32), np.array(sq)


def cluster_sums_loop(y, labels, k, slice_len=1024):
    y = np.asarray(y, dtype=np.float64).reshape(len(labels), -1)
    counts, sums = [0] * k, [[0.0] * y.shape[1] for _ in range(k)]
    for t0 in range(0, len(labels), slice_len):
        part = [[0.0] * y.shape[1] for _ in range(k)]
        for t in range(t0, min(t0 + slice_len, len(labels))):
            c = int(labels[t])
            if 0 <= c < k:
                counts[c] += 1
                for j in range(y.shape[1]):
                    part[c][j] = part[c][j] + float(y[t, j])
        for c in range(k):
            for j in range(y.shape[1]):
                sums[c][j] = sums[c][j] + part[c][j]
    return np.array(counts, dtype=np.int64), np.array(sums, dtype=np.float64).reshape(k, y.shape[1])


def state_loop(label, n_states, state_map):
    label = int(label)
    if state_map is None:
        return label if 0 <= label < n_states else -1
    if not 0 <= label < len(state_map):
        return -1
    s = int(state_map[label])
    return s if 0 <= s < n_states else -1


def transition_counts_loop(labels, lag, n_states, state_map=None):
    out = np.zeros((n_states, n_states), dtype=np.int64)
    for t in range(len(labels) - lag):
        a, b = state_loop(labels[t], n_states, state_map), state_loop(labels[t + lag], n_states, state_map)
        if a >= 0 and b >= 0:
            out[a, b] += 1
    return out


def label_counts_loop(labels, bounds, n_states, state_map=None):
    out = np.zeros((len(bounds) - 1, n_states), dtype=np.int64)
    for s in range(len(bounds) - 1):
        for t in range(int(bounds[s]), int(bounds[s + 1])):
            a = state_loop(labels[t], n_states, state_map)
            if a >= 0:
                out[s, a] += 1
    return out


# ---- frames for the assignment ---------------------------------------------------------------------------------------------------------------------------

# d -> [(y, c0, c1, the specification's label, the contracted evaluation's label)]
_FMA_HEX = {
    3: [
        (["-0x1.8d8480a2ac896p-4", "-0x1.ccf9556a807c0p-4", "-0x1.24ddbdb1c2b4ap+0"],
         ["-0x1.e8abd7e5d2889p-2", "-0x1.505970c30f50cp+0", "0x1.c4ed39831c5b5p-1"],
         ["0x1.c33c1e514feadp-1", "0x1.b5a6948e830e8p+0", "0x1.99e0271b2e20cp-5"], 1, 0),
        (["-0x1.d680a13834fb5p-1", "-0x1.6b1e02b0e85fbp-1", "0x1.0f867ad6fda48p-1"],
         ["0x1.e893d1ab4d365p-3", "0x1.3a684fe240e60p-1", "-0x1.ad02d66058c62p-1"],
         ["0x1.2916e7036b1b5p-3", "0x1.2afa55613e465p+0", "-0x1.8aed79a92c8bcp-6"], 1, 0),
        (["-0x1.268012edc238ep-3", "0x1.6fb2b9842af93p+0", "-0x1.418cc6d88eba0p-6"],
         ["0x1.16e38b4d6908dp+0", "0x1.87f03b54b406dp-6", "0x1.928f6f08efd1bp-2"],
         ["-0x1.ee5b276776275p-3", "-0x1.e6effd02f8c79p-2", "-0x1.5382e76638db0p-3"], 1, 0),
        (["0x1.e66e94bb00548p-3", "0x1.70e851f77aa15p-1", "-0x1.17168a595d394p-1"],
         ["-0x1.28b69d2023353p+0", "0x1.80d5c67c30f00p+0", "0x1.d10f269a0dd57p-1"],
         ["-0x1.079b0b1f99a74p+0", "-0x1.07bbc0811b668p+0", "-0x1.398a734d11090p-1"], 1, 0),
        (["0x1.22911ca1cae9ep-2", "-0x1.734e845a6664ap-4", "0x1.79b602c0120a7p+0"],
         ["-0x1.4742a34db9242p-2", "0x1.1dae9567e859ap+0", "-0x1.f07d88c599067p-6"],
         ["0x1.7dd46892bb39bp+0", "-0x1.65eaee4e8fd73p+0", "0x1.0899b0630d974p-1"], 1, 0),
        (["0x1.d1afef20f8e4cp-1", "0x1.5cfc947474ff0p-5", "0x1.8e3910b64efb4p+0"],
         ["-0x1.28e82564a941fp+0", "-0x1.42759332478e2p-5", "-0x1.6c37bc7c0e839p-5"],
         ["0x1.610bbe2709a9bp-3", "-0x1.98000d98904a0p+0", "-0x1.65858b0ac958ap-2"], 1, 0),
    ],
    17: [
        (["-0x1.a51fea8020edep-2", "0x1.285853f401878p+0", "-0x1.3251e82c32b1ep-2", "-0x1.0b5091786cebfp-1", "0x1.e219677622800p-6", "0x1.83c83a253b0a4p+0", "0x1.991912b58ad89p+0", "-0x1.51f4fa9b893dap-1", "0x1.db81ce0610f5dp-2", "-0x1.5efd95f3d5f37p+0", "-0x1.42f32e10c4ce2p-1", "-0x1.b32b8312b0478p-1", "-0x1.8ece76048ac7cp+0", "-0x1.ad06f4e5827bcp+0", "-0x1.48eea7eb12bdap+0", "0x1.6216eade32f4dp-1", "0x1.20a1726bbb8d6p-2"],
         ["-0x1.1b55b52d8ab14p+0", "0x1.5451af38716e1p+0", "0x1.0e607da991e86p-7", "-0x1.3e16000e1d537p+0", "0x1.10edd8faa7d1fp+0", "0x1.883bf8cd9f670p-2", "0x1.5b27a60f6e468p-1", "0x1.7ad9f1821c02ap-3", "0x1.d7b10625c9105p-1", "0x1.ca077bf6f0886p-2", "-0x1.294d9f64ebae3p+0", "0x1.99dcedef9c20ap-1", "-0x1.a5f4b58ad9ce6p-5", "-0x1.7737204a4094ep+0", "0x1.57d1d0ffa1facp+0", "0x1.b84a0dab1ac76p-1", "0x1.dce0135c92ae7p-2"],
         ["0x1.7c494d030274cp-4", "-0x1.7ee13a574a451p+0", "-0x1.1ffddb3766f8cp-1", "0x1.6e2d0de99f224p+0", "0x1.973cb2d06196fp-3", "0x1.475bb9228025bp+0", "0x1.57d104215f931p+0", "0x1.ca88d25326745p-5", "0x1.85f93936bcd0dp-1", "-0x1.fdd347f5395bcp-1", "0x1.5ecf8f71c7d62p-1", "-0x1.253634402ef99p+0", "0x1.8b3f93471468cp-2", "-0x1.055c348e4c518p-1", "-0x1.3008ac9a84a8fp+1", "0x1.c361989b13e39p-2", "-0x1.e5187b26e2b0fp-2"], 1, 0),
        (["-0x1.b669ac21aba60p-1", "-0x1.493860bcd240cp-1", "-0x1.17e8d9ee601a0p-5", "0x1.11b52d11e70b9p-2", "-0x1.972fa5619421ap+1", "0x1.7ddad5f461ad2p+0", "-0x1.d406a1885c109p+0", "-0x1.67e4310531212p-1", "0x1.27c2af0c2d35ap-1", "0x1.f4a986c2f1f50p-1", "-0x1.f2c65f0df1cb8p-4", "-0x1.1b7aeef917bc8p+1", "-0x1.176451f93d808p-6", "0x1.4d02f3505e7fcp+1", "-0x1.943876c6a200cp+0", "-0x1.1a0e6c797b1a2p+0", "-0x1.c92014511de2cp-1"],
         ["0x1.a33a0f54b1c7fp+0", "-0x1.a03df4fa3db34p-1", "-0x1.ed33c256c3b34p+0", "0x1.83c9bb491be72p+0", "-0x1.62dfc4b05034fp+0", "0x1.b88fab78b2badp+0", "-0x1.a164a0f77a983p-10", "0x1.8bd924d0ffbd9p-4", "-0x1.687dea6e98168p-2", "0x1.170353e5c98e2p+1", "-0x1.1150e2f65ec5cp+1", "-0x1.a6eef80d4d4e5p+0", "0x1.fd2226ba27379p-2", "0x1.20546b06b7db2p-2", "0x1.86842fa07aaf0p-3", "-0x1.f98070b9dcfcfp+0", "-0x1.9b5b287ae5a57p-2"],
         ["0x1.cfacb0552ea95p-2", "-0x1.156efd5b605a4p+0", "0x1.e9b21dae438d7p+0", "-0x1.0337df52784dbp-4", "-0x1.9ff0be03bcf4ap-1", "-0x1.fc5dbcc300b9dp-2", "-0x1.760e2135d0bf2p-1", "-0x1.15e09b83b7a3cp-2", "-0x1.479829914936ap+0", "-0x1.25fc523bcc3a5p+0", "0x1.4e9da24b9b7e7p+0", "-0x1.183bbf968fa66p-2", "-0x1.e7611729917b6p-1", "0x1.0c3b2b2a3ac20p+0", "-0x1.fa245ab76c4b2p+0", "-0x1.09a30248fd692p-2", "-0x1.0bb8c913d3493p-2"], 1, 0),
        (["0x1.114a8c880a596p-1", "-0x1.1c10170cd3dd0p-4", "-0x1.04f52aef828b4p+0", "-0x1.0a8a4e379b359p+0", "-0x1.94b4c2c2248c8p+0", "0x1.e92a13efaa3bdp-1", "-0x1.514882f1b73ecp-2", "0x1.2ac68efa9a5a0p-4", "0x1.2b65ccd68679ap+0", "0x1.4e7fa080e32b6p-1", "-0x1.4ff88522724a9p-1", "0x1.aa9518e1b2742p+0", "-0x1.c5166ca989c44p-3", "-0x1.da70a8b0b9157p+0", "-0x1.0f37a3e17b811p+1", "-0x1.b349751f51355p-2", "0x1.237c900a5dc0cp-3"],
         ["-0x1.8ca6cdc4b567ep-1", "-0x1.a2b974118e634p-5", "-0x1.da264cd2dabd2p-1", "-0x1.6d2fd61719fadp+0", "-0x1.885e0d19b5aa3p+1", "0x1.07a721454be82p+0", "-0x1.f5f1e8a082f8fp+0", "-0x1.7a3df139445e6p-1", "-0x1.3bf3adaf47950p+0", "0x1.bb862a053ffefp+0", "-0x1.6c474587e9745p-2", "0x1.1eb0b87b4602ep+0", "-0x1.38b5f413f2f0dp-2", "0x1.b96bbfd807ad4p-2", "-0x1.8b54f8c601c70p-3", "-0x1.64cee260a7605p-5", "0x1.1fc211a7c24cap-3"],
         ["0x1.cf094834ffca0p+0", "-0x1.094a062be18c3p-2", "0x1.73e01fe9e4eb0p-3", "-0x1.25947a82eb4d0p+0", "-0x1.9e44a3a0e134dp-1", "0x1.f413a1246bfadp-1", "-0x1.b296dea727269p-1", "-0x1.4513b9deadefep+0", "0x1.b97023b1fa9d4p+0", "-0x1.c1c95f3b2412ap-1", "-0x1.299efd7cd783bp+0", "-0x1.8cf5efc8da135p-1", "0x1.e0f91053cbd04p+0", "-0x1.89f03390b8316p-1", "-0x1.34cd60110d299p-2", "0x1.5b68793a5802ap-5", "0x1.71c32a25096e6p-2"], 1, 0),
        (["-0x1.f5403b5563f00p-3", "-0x1.83c293c5d5bf6p-1", "0x1.e2e9ef950690ep+0", "-0x1.1105f640b1a02p+1", "-0x1.6642fdb048400p-11", "0x1.6f0836db2932dp+0", "-0x1.aa2757de90094p-2", "0x1.3da933547d51fp+0", "-0x1.1f20146316734p+0", "-0x1.1ea239424fdc0p-6", "-0x1.32990d798b34ap+0", "0x1.cc5ad88381d76p-2", "0x1.c157461bc9213p-1", "0x1.1b1cc1aed50f9p-1", "0x1.09508459309b0p-1", "0x1.2238e391cfc6cp-1", "0x1.79e8c52a326c8p-3"],
         ["-0x1.fb2dc42fdf42ap-3", "0x1.e53e2a6005ff1p-2", "0x1.9f2119e3477d5p+0", "0x1.1c4af3bd2d89ap-2", "0x1.00091f2a5e0b8p+0", "0x1.f58e76a414945p-6", "-0x1.257412f491bfbp-2", "0x1.26e3496647e22p+0", "0x1.cb0a453d1a8a4p-1", "-0x1.35be71b4169e7p+0", "-0x1.9e0238de32151p+0", "0x1.27e18e5b1970dp-3", "0x1.a2bdbe9154f7dp-1", "0x1.fb4205dd7774cp-1", "-0x1.fba9fd5861184p-1", "-0x1.f324852be7eb4p-2", "-0x1.c04c72eadbad5p-1"],
         ["0x1.14c36df884149p-4", "0x1.592bc9ffcee3ep+0", "0x1.0cc45c0f91ea4p-2", "-0x1.8e0e8f628d042p-1", "0x1.e5fec751bac93p-4", "-0x1.f095f1b994146p-3", "-0x1.5e71ee1cb47e3p-2", "0x1.0420f0b359e86p+0", "-0x1.8e93386661a5bp+0", "-0x1.e52f0d7a5f02ep-2", "-0x1.d99b1b061c0edp-4", "0x1.2cf5a841e6db9p-2", "-0x1.2a60f07bab1cfp-1", "-0x1.25893dbe73d3ap+0", "0x1.307372fa210bep-2", "0x1.36e4f96eb7c51p-1", "-0x1.565386c62fa62p+0"], 0, 1),
        (["-0x1.43dcd57e1b25ap+0", "0x1.3e49d80f49b80p-6", "-0x1.62277fb9f45b8p+0", "0x1.179a78b9cebc1p+0", "0x1.0388a0961c941p+1", "0x1.142bf9bb6ab56p-1", "0x1.20d340afd4e74p+1", "0x1.509e62cf2206dp+0", "-0x1.28b1b41ac0ba6p+0", "0x1.f6df949a2a5a2p+0", "0x1.261cafb04b1d0p-1", "-0x1.551dc885ef770p-3", "0x1.5ca93e5717023p+0", "0x1.99f42cd369140p-6", "0x1.144015e6e54d8p+0", "-0x1.0cad1fdff7690p-3", "0x1.2fd057f34016ep-3"],
         ["-0x1.aac5dc46135f8p-1", "0x1.b2d7db494e806p+0", "-0x1.058fbf8d8d403p+1", "0x1.1628f0164b249p+0", "0x1.74085c1308468p-2", "-0x1.3a77ee677670ap-3", "0x1.0a15ad50c1c81p+1", "-0x1.5cef6567cbc3ep+0", "0x1.e9c84a70924cfp-4", "0x1.b1172df0b7d62p-1", "-0x1.359c0a14eddadp-3", "0x1.de181d9170113p+0", "0x1.108b103f3ccf2p-2", "0x1.2964b94ab0f91p+1", "0x1.9f16935533894p+0", "0x1.d5844aa78eeadp-1", "-0x1.3230876513a67p+0"],
         ["-0x1.1f32d46e9fa5ep+0", "0x1.8daf8ba394ad2p-4", "-0x1.ad3f8c43b85ecp-2", "-0x1.e5532c0613ec5p+0", "-0x1.096ac28bacf4fp-1", "0x1.0bb21c1275c18p+0", "0x1.cb281bf32ff6fp+0", "0x1.3774ae06bff03p-1", "0x1.2d40d29da853bp-1", "0x1.777fbccffed74p+0", "0x1.2830bebbbc1a5p-2", "-0x1.78fda8aaaf435p-4", "0x1.46310b12949c4p-4", "-0x1.91926118f6c29p-3", "-0x1.50e41a04a96c5p+0", "-0x1.044772b6b711bp-3", "0x1.df77512499c1bp+0"], 1, 0),
        (["0x1.3d1f153ae63c0p+0", "0x1.0c715bae17800p-11", "-0x1.7b3a3d1f7096ep+0", "0x1.31654a07afb4cp-1", "-0x1.5b79badbddb55p+0", "-0x1.1210810f53c2fp+0", "-0x1.b9cb1a5825d40p+0", "0x1.6ea57da8944b6p+0", "0x1.0c73b8101b298p-4", "-0x1.b50565712ee71p-1", "-0x1.33a78da253c3ep+0", "0x1.370949f2fa835p+0", "0x1.406abc4180104p-2", "0x1.849e0c9d13ea4p+0", "-0x1.72e9da6149822p+0", "0x1.efd7cc82475c4p-3", "-0x1.7bcdef5b9336ap-1"],
         ["0x1.fc0cbade4f943p+0", "0x1.a9b2dd5ddff68p-2", "-0x1.9f0d5ab637598p-2", "0x1.a766ff606e18fp+0", "0x1.94cc8c01aed02p+0", "0x1.44003cb8d346fp-2", "-0x1.0002b95309f2dp-1", "0x1.9f24132279844p-1", "0x1.3deaf23c13a77p-2", "-0x1.5f648cc2709b3p+1", "0x1.f5d0c78b1088dp-2", "0x1.da8b754b74218p-1", "-0x1.3c9adfbab3f87p-1", "0x1.161f07468165cp-2", "-0x1.f136935a6a48cp-1", "0x1.cba6ac50e9b95p-3", "-0x1.95febb302e8dbp-1"],
         ["-0x1.4349da551cc85p+0", "0x1.14710c9015420p+0", "0x1.99f25a44c2851p-5", "0x1.4b67dd7b809bap-2", "-0x1.4ee881c279734p+0", "-0x1.3e82d5d044a10p-2", "-0x1.c95e5745ff5c0p-1", "0x1.17123d81aa8b9p-1", "0x1.2bf283b6779dcp-1", "0x1.adcd1d5a0921ep-2", "-0x1.8d40febd3b8c9p+0", "-0x1.5de17bf96f3f5p-1", "-0x1.c89daf95bb02ap-2", "0x1.9909960bb8650p-1", "-0x1.37017121bae32p-2", "-0x1.6f8c6e027912bp+0", "0x1.4eddd6cd377ddp-1"], 1, 0),
    ],
}


@functools.lru_cache(maxsize=None)
def fma_cases(d: int):
    """[(y float64 [1, d], centers float64 [2, d], the specification's label, the contracted evaluation's label)]"""
    un = lambda h: np.array([float.fromhex(v) for v in h], dtype=np.float64)
    return [(_frozen(un(y)[None, :]), _frozen(np.stack([un(c0), un(c1)])), ls, lf) for y, c0, c1, ls, lf in _FMA_HEX[d]]


# exact ties: every coordinate a small integer or a half, so every operation is exact and the lowest index must win
TIE_CENTERS = _frozen(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0]]))  # (the last one repeats the first)
TIE_FRAMES = _frozen(np.array([[0.5, 0.5], [0.5, 0.0], [1.0, 0.5], [0.5, 1.0], [0.0, 0.5], [0.0, 0.0], [1.0, 1.0], [2.5, 0.5], [0.5, -3.0]]))
TIE_LABELS = np.array([0, 0, 1, 2, 0, 0, 3, 1, 0], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def projection_rows(T: int, d: int, seed: int = 0) -> np.ndarray:
    """float64 [T, d]: rows around a few clumps, columns of different scales (a kinetic map scales its columns by the eigenvalues)."""
    rng = np.random.RandomState(seed + 31 * d + T)
    clumps = rng.randn(5, d) * 2.0
    scale = np.array([1.0, 0.3, 0.05])[np.arange(d) % 3]
    return _frozen((clumps[rng.randint(5, size=T)] + 0.5 * rng.randn(T, d)) * scale[None, :])


def centers_for(y: np.ndarray, k: int, seed: int = 0) -> np.ndarray:
    """float64 [k, d]: rows of ``y`` where it has enough, else random points of its scale."""
    rng = np.random.RandomState(seed + k)
    if y.shape[0] >= k:
        return np.array(y[rng.choice(y.shape[0], k, replace=False)])
    return rng.randn(k, y.shape[1]) * (np.abs(y).max() + 1.0)


def labels_with_outliers(T: int, n: int, seed: int = 0) -> np.ndarray:
    """int32 [T]: labels in [0, n) with -1, n, n + 5 and a large negative value strewn in."""
    rng = np.random.RandomState(seed + T + 7 * n)
    lab = rng.randint(n, size=T).astype(np.int32)
    bad = rng.rand(T) < 0.1
    lab[bad] = rng.choice([-1, n, n + 5, -2**31], size=int(bad.sum()))
    return lab


# ---- a block-structured transition matrix ---------------------------------------------------------------------------------------------------------------------

MIN_PCCA_GAP = 0.05  # lambda_2 - lambda_3 of the block fixture, at least


def block_counts(seed: int = 0, coupling: float = 2.0) -> np.ndarray:
    """Symmetric counts [9, 9]: three blocks of three states (weights 3 : 2 : 1) coupled weakly."""
    rng = np.random.RandomState(seed)
    c = np.full((9, 9), coupling)
    for b, w in enumerate((300.0, 200.0, 100.0)):
        c[3 * b : 3 * b + 3, 3 * b : 3 * b + 3] = w * (1.0 + 0.2 * rng.rand(3, 3))
    return np.round((c + c.T) / 2.0)


# ---- the meter fixture: psi hopping between three wells -----------------------------------------------------------------------------------------------------------

WELLS, DWELL, NOISE = (0.6, 2.6, -1.6), 50, 0.1
REFERENCE_T, CHAIN_T = 3000, 400
METER_KW = dict(k=8, n_metastable=3, msm_lag=5, traj_lag=2, n_steps=10, lag=tc.METER_LAG)


def hopping_states(T: int, seed: int) -> np.ndarray:
    rng = np.random.RandomState(seed)
    s = np.empty(T, dtype=np.int64)
    s[0] = rng.randint(3)
    for t in range(1, T):
        s[t] = (s[t - 1] + 1 + rng.randint(2)) % 3 if rng.rand() < 1.0 / DWELL else s[t - 1]
    return s


def hopping_frames(mol: dict, T: int, seed: int) -> np.ndarray:
    """float32 [T, 10, 3]: the Ala-Gly dipeptide with psi of ALA turned by a well of `hopping_states` plus noise, phi of GLY by noise."""
    rng = np.random.RandomState(seed + 991)
    psi = np.asarray(WELLS)[hopping_states(T, seed)] + NOISE * rng.randn(T)
    pos = np.repeat(np.asarray(mol["pos"].numpy(), dtype=np.float64)[None], T, axis=0)
    pos = tc._rotate(pos, 1, 3, (4, 5, 6, 7, 8, 9), psi)
    pos = tc._rotate(pos, 5, 6, (7, 8, 9), NOISE * rng.randn(T))
    pos += 0.2 * rng.randn(T, 1, 3)
    return _frozen(pos.astype(np.float32))


def meter_fixture(mol: dict, device):
    """(reference frames [REFERENCE_T, 10, 3] as a CPU tensor, two batches of three chains of CHAIN_T frames on ``device``)."""
    batches = []
    for b in range(2):
        frames = [hopping_frames(mol, CHAIN_T, 700 + 10 * b + c) for c in range(3)]
        block = torch.from_numpy(np.stack([np.array(f.transpose(1, 0, 2), order="C") for f in frames])).to(device)
        batches.append([{"dataset_label": "m", "atom_type_index": mol["atom_type_index"], "xhat_traj": block[c]} for c in range(3)])
    return torch.from_numpy(np.array(hopping_frames(mol, REFERENCE_T, 500))), batches


INTEGER_OUTPUTS = ("metastable_map", "transition_counts", "steps", "num_frames", "nonfinite_frames", "unassigned_frames")


def meter_outputs(directory) -> dict:
    """Every array of every ``.npz`` under ``directory`` as ``"<file>/<name>"`` -> array."""
    import os

    out = {}
    for name in sorted(os.listdir(directory)):
        if name.endswith(".npz"):
            z = np.load(os.path.join(directory, name))
            out.update({f"{name}/{k}": z[k] for k in z.files})
    return out


def compare_outputs(a: dict, b: dict) -> dict:
    """Two `meter_outputs`: asserts the same arrays, every integer array equal; returns the largest absolute difference of the centres,
    of the inertia and of every other float array (NaN and infinities in the same places)."""
    assert sorted(a) == sorted(b)
    worst = {"centers": 0.0, "inertia": 0.0, "other_floats": 0.0}
    for key in a:
        x, y = a[key], b[key]
        assert x.shape == y.shape and x.dtype == y.dtype, key
        name = key.split("/")[1]
        if x.dtype.kind in "iu":
            assert np.array_equal(x, y), key
            continue
        assert name not in INTEGER_OUTPUTS, key
        fin = np.isfinite(x)
        assert np.array_equal(fin, np.isfinite(y)) and np.array_equal(x[~fin], y[~fin], equal_nan=True), key
        diff = float(np.abs(x[fin] - y[fin]).max()) if fin.any() else 0.0
        slot = name if name in worst else "other_floats"
        worst[slot] = max(worst[slot], diff)
    return worst


def measure_stability(run, draws: int = 16) -> dict:
    """``run(shift)`` runs the host meter with ``shift(proj)`` applied to every projection and returns (`meter_outputs`, the microstate
    labels of every trajectory).  The projections are moved by +-`_tica_cases.METER_TOLERANCE["tic01"]` with random signs, ``draws`` times;
    every label and every integer output must stay (asserted); returns the largest change of the float outputs (`compare_outputs`)."""
    eps = tc.METER_TOLERANCE["tic01"]
    base, base_labels = run(lambda proj: proj)
    worst = {"centers": 0.0, "inertia": 0.0, "other_floats": 0.0}
    for seed in range(draws):
        rng = np.random.RandomState(1000 + seed)
        moved, labels = run(lambda proj: proj + np.where(rng.rand(*proj.shape) < 0.5, -eps, eps))
        assert len(labels) == len(base_labels) and all(np.array_equal(p, q) for p, q in zip(labels, base_labels)), seed
        for k, v in compare_outputs(base, moved).items():
            worst[k] = max(worst[k], v)
    return worst


# The largest changes `measure_stability` saw on this fixture with 16 draws (test_msm_host.py repeats the measurement and holds the
# constants to it within a factor 2).  Every float output but the centres and the inertia is computed from integers (counts) alone and did
# not move: ten times the observed change is 0, so the device path is compared with the host path for equality there.
OBSERVED = {"centers": 1.64e-10, "inertia": 1.23e-8, "other_floats": 0.0}
TOLERANCE = {k: 10.0 * v for k, v in OBSERVED.items()}
