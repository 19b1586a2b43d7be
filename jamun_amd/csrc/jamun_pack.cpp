// jamun_pack.cpp — checkpoint tensors to device weight layouts: constant folding, the MFMA-ordered packing of every conv / node-update
// kernel's weights, the f16 hi + lo splits and their balancing scales.
#include <cmath>
#include <cstring>

#include "jamun_host.h"

namespace {

// ---- packed conv problem ------------------------------------------------------------------------
struct UEntry {
  int type;      // JAMUN_T_*
  int cross;     // 1 for the cross-product half of an X1C block
  int xoff;      // offset of the channel's first float inside a node feature row
  int64_t wbase; // offset of W row (u, :) inside the flat tensor-product weight vector
  double scale;  // path coefficient * CG factor * input noise scaling
};
struct UBlock {
  int type;
  std::vector<UEntry> e;  // nu entries (even)
};

// fp32 -> IEEE binary16, round to nearest even (the device side uses v_cvt_pk_f16_f32 in the default rounding mode); values
// beyond the f16 range do not occur (the caller scales into [-2^14, 2^14])
uint16_t f32_to_f16_rne(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);  // >= 65536 (or inf / nan): inf
  if (x < 0x38800000u) {                                     // below the smallest normal half (2^-14): subnormal or zero
    if (x < 0x33000000u) return (uint16_t)sign;              // < 2^-25: rounds to zero
    const int e = (int)(x >> 23);                             // biased exponent, 102 .. 112
    const uint32_t mant = (x & 0x7fffffu) | 0x800000u;        // 24-bit significand
    const int shift = 126 - e;                                // result = mant >> shift, in units of 2^-24
    const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
  const uint32_t mant = x & 0x7fffffu, e = (x >> 23) - 112u;  // half exponent field 1 .. 30
  uint32_t h = (e << 10) | (mant >> 13);
  const uint32_t rem = mant & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;     // (a carry into the exponent is the correct result)
  return (uint16_t)(sign | h);
}
float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  float out;
  if (e == 0) {
    out = std::ldexp((float)m, -24);
    if (sign) out = -out;
    return out;
  }
  const uint32_t x = sign | ((e == 31 ? 255u : e + 112u) << 23) | (m << 13);
  std::memcpy(&out, &x, 4);
  return out;
}

// value -> (hi, lo) halves with hi = rne16(v), lo = rne16(v - hi)
inline void split_f16(double v, uint16_t& hi, uint16_t& lo) {
  const float f = (float)v;
  hi = f32_to_f16_rne(f);
  lo = f32_to_f16_rne(f - f16_to_f32(hi));
}

int pow2_above(double v) { int ex = 0; if (v > 0 && std::isfinite(v)) std::frexp(v, &ex); return std::max(-40, std::min(40, ex)); }  // v < 2^ex

}  // namespace

// eight values -> one lane's fragment of an f16 MFMA, hi and lo planes
static void pack8(const double (&v)[8], float4& hi, float4& lo) {
  uint32_t h[4], l[4];
  for (int i = 0; i < 4; ++i) {
    uint16_t h0, l0, h1, l1;
    split_f16(v[2 * i], h0, l0);
    split_f16(v[2 * i + 1], h1, l1);
    h[i] = (uint32_t)h0 | ((uint32_t)h1 << 16);
    l[i] = (uint32_t)l0 | ((uint32_t)l1 << 16);
  }
  std::memcpy(&hi, h, 16);
  std::memcpy(&lo, l, 16);
}

std::vector<double> noise_mlp(const jamun_model& m, const std::string& prefix, int k, double c_noise) {
  // Linear(1->k) . SELU . Linear(k->k)   (src/jamun/model/noise_conditioning.py:33-37)
  const auto& w0 = m.get(prefix + ".0.weight", k);
  const auto& b0 = m.get(prefix + ".0.bias", k);
  const auto& w2 = m.get(prefix + ".2.weight", (int64_t)k * k);
  const auto& b2 = m.get(prefix + ".2.bias", k);
  const double alpha = 1.6732632423543772848170429916717, scale = 1.0507009873554804934193349852946;
  std::vector<double> h(k), out(k);
  for (int i = 0; i < k; ++i) {
    double z = (double)w0[i] * c_noise + (double)b0[i];
    h[i] = scale * (z > 0 ? z : alpha * (std::exp(z) - 1.0));
  }
  for (int o = 0; o < k; ++o) {
    double s = b2[o];
    for (int i = 0; i < k; ++i) s += (double)w2[(size_t)o * k + i] * h[i];
    out[o] = s;
  }
  return out;
}

namespace {

// K-slices are ranges of the hidden index k (hidden units + bias row); each is processed in k-subgroups of
// ksub or ksub-1 hidden units (the two sizes the conv kernel is instantiated for).  any_size: the wide kernel (k_conv_wide) forms
// k-subgroups of any size 1..ksub — a slice is cut into ceil(size / ksub) near-equal subgroups; slices may be empty (n_k < n_slices).
std::vector<std::pair<int, int>> k_subgroups(int n_k, int n_slices, int ksub, std::vector<int>& slice_first_sub, bool any_size) {
  std::vector<std::pair<int, int>> subs;  // (k0, ks)
  slice_first_sub.assign(n_slices + 1, 0);
  const int base = n_k / n_slices, rem = n_k % n_slices;
  int k = 0;
  for (int s = 0; s < n_slices; ++s) {
    const int size = base + (s >= n_slices - rem ? 1 : 0);
    slice_first_sub[s] = (int)subs.size();
    if (size == 0) continue;
    const int n_sub = (size + ksub - 1) / ksub;
    const int lo = size / n_sub, n_hi = size % n_sub;  // n_hi subgroups of lo+1, the rest of lo
    if (!any_size && (lo + (n_hi ? 1 : 0) > ksub || lo < ksub - 1 || (lo < 1)))
      throw Err(JAMUN_ERR_INVALID, "cannot split a K-slice of " + std::to_string(size) + " hidden units into groups of " +
                                       std::to_string(ksub - 1) + "/" + std::to_string(ksub));
    for (int i = 0; i < n_sub; ++i) {
      const int ks = lo + (i < n_hi ? 1 : 0);
      subs.push_back({k, ks});
      k += ks;
    }
  }
  slice_first_sub[n_slices] = (int)subs.size();
  return subs;
}

// (wide = true: the chunking of k_conv_wide — k-subgroups of 1..ksub, an even number of weight groups per chunk)
ConvProblemDev pack_problem(DevArena& mem, const std::vector<UBlock>& blocks, int planes, int G, int n_slices, int ksub,
                            const std::vector<float>& W3, const std::vector<float>& b3, int hidden, bool wide = false) {
  ConvProblemDev P;
  P.planes = planes;
  P.nt = (G + 31) / 32;
  const int NT = P.nt;
  std::vector<int> first_sub;
  const auto subs = k_subgroups(hidden + 1, n_slices, ksub, first_sub, wide);
  std::vector<int4> chunks;
  std::vector<int> sp(n_slices + 1, 0);
  int64_t gofs = 0;  // in weight groups (4 K-steps x NT tiles x 64 lanes x float)
  for (int s = 0; s < n_slices; ++s) {
    sp[s] = (int)chunks.size();
    for (int si = first_sub[s]; si < first_sub[s + 1]; ++si)  // k-subgroup major: the staged h~ records are reused by the u-blocks
      for (size_t b = 0; b < blocks.size(); ++b) {
        const int nu = (int)blocks[b].e.size(), k0 = subs[si].first, ks = subs[si].second;
        int ng = (ks * nu / 2 + 3) / 4;
        if (wide) ng = (ng + 1) & ~1;  // (k_conv_wide consumes weight groups in pairs: zero weights and zeroed A rows pad a chunk)
        chunks.push_back(make_int4((int)b, k0 | (ks << 16), (int)gofs, ng));
        gofs += ng;
      }
  }
  sp[n_slices] = (int)chunks.size();
  if (gofs * NT * 64 > (int64_t)0x7fffffff) throw Err(JAMUN_ERR_INVALID, "packed conv weights too large");
  std::vector<float4> wp((size_t)gofs * NT * 64, make_float4(0.f, 0.f, 0.f, 0.f));
  int64_t Ktot = 0;
  for (const int4& cd : chunks) {
    const UBlock& B = blocks[cd.x];
    const int nu = (int)B.e.size(), k0 = cd.y & 0xffff, ks = cd.y >> 16;
    Ktot += (int64_t)cd.w * 8;
    for (int g = 0; g < cd.w; ++g)
      for (int nt = 0; nt < NT; ++nt)
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, c = lane & 31, col = nt * 32 + c;
          float v[4] = {0.f, 0.f, 0.f, 0.f};
          for (int st = 0; st < 4; ++st) {
            const int kidx = 2 * (4 * g + st) + hh;
            if (kidx >= ks * nu) continue;
            const int kk = kidx / nu, ul = kidx % nu, k = k0 + kk;
            const UEntry& ue = B.e[ul];
            if (k <= hidden && col < G && ue.scale != 0.0) {
              const int64_t p = ue.wbase + col;
              const double w = (k < hidden) ? (double)W3[(size_t)p * hidden + k] : (double)b3[p];
              v[st] = (float)(w * ue.scale);
            }
          }
          wp[((size_t)(cd.z + g) * NT + nt) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
  }
  P.K = Ktot;
  std::vector<int4> ub;
  std::vector<int> lx;
  int xw = 1;
  for (const UBlock& B : blocks) {
    int lo = 1 << 30, hi = 0;
    const int per = (B.type == JAMUN_T_X0 || B.type == JAMUN_T_X0V) ? 1 : 3;
    for (const UEntry& e : B.e)
      if (e.scale != 0.0) { lo = std::min(lo, e.xoff); hi = std::max(hi, e.xoff + per); }
    if (hi == 0) { lo = 0; hi = per; }
    ub.push_back(make_int4(B.type, (int)B.e.size(), lo, hi - lo));
    xw = std::max(xw, hi - lo);
    for (int lane = 0; lane < 64; ++lane) {
      int v = 0;
      if (lane < (int)B.e.size() && B.e[lane].scale != 0.0) v = (B.e[lane].xoff - lo) | (B.e[lane].cross ? JAMUN_XOFF_CROSS : 0);
      lx.push_back(v);
    }
  }
  P.xw = xw;
  P.wpack = mem.upload(wp); P.chunks = mem.upload(chunks); P.slice_ptr = mem.upload(sp); P.ublk = mem.upload(ub); P.lane_xoff = mem.upload(lx);
  return P;
}

void pad_even(UBlock& b) {
  if (b.e.size() % 2) b.e.push_back(UEntry{b.type, 0, 0, 0, 0.0});
}

void build_layer_common(DevArena& mem, const jamun_model& m, const std::string& prefix, const std::vector<InBlock>& in_blocks, const std::vector<double>& s_in,
                        LayerDev& L, int in0, int in1, bool wide = false) {
  const jamun_hparams& hp = m.hp;
  const int mul0 = hp.mul0, mul1 = hp.mul1, H = hp.edge_attr_dim;
  // ---- radial MLP first layer: split into the constant bonded part and the radial part
  const auto& W1 = m.get(prefix + ".gated_conv.f.f.radial_nn.0.weight", (int64_t)H * H);
  const auto& b1 = m.get(prefix + ".gated_conv.f.f.radial_nn.0.bias", H);
  const int nb = H / 2, nr = (H + 1) / 2;
  const auto& Eb = m.get("embed_bondedness.weight", 2 * nb);
  std::vector<float> w1r((size_t)H * nr), cmask(2 * (size_t)H);
  for (int k = 0; k < H; ++k) {
    for (int r = 0; r < nr; ++r) w1r[(size_t)r * H + k] = W1[(size_t)k * H + nb + r];  // [basis][hidden]: lane = hidden unit
    for (int mk = 0; mk < 2; ++mk) {
      double s = b1[k];
      for (int c = 0; c < nb; ++c) s += (double)W1[(size_t)k * H + c] * Eb[(size_t)mk * nb + c];
      cmask[(size_t)mk * H + k] = (float)s;
    }
  }
  L.w1r_h = w1r;
  L.cmask_h = cmask;
  {
    // static bound of |h~| = |SiLU(c_mask + W1[:, radial part] . radial(d))| over the layer: the Gaussian basis values are
    // positive and sum to at most sqrt(pi) / 1.12 < 1.6 at any distance, |SiLU(z)| <= max(|z|, 0.2785); the bias row is 1
    double hm = 1.0;
    for (int k = 0; k < H; ++k) {
      double wm = 0;
      for (int r = 0; r < nr; ++r) wm = std::max(wm, std::fabs((double)W1[(size_t)k * H + nb + r]));
      const double z = std::max(std::fabs((double)cmask[k]), std::fabs((double)cmask[(size_t)H + k])) + 1.6 * wm;
      hm = std::max(hm, z);
    }
    L.dg.hmax2 = (float)(2.0 * hm * 1.0001);
  }

  // ---- o3.Linear skip (in -> hidden) and self-interaction (hidden -> hidden)  (_interaction.py:23-30)
  int64_t n_skip = 0;
  for (auto& ib : in_blocks) n_skip += (int64_t)ib.mul * (ib.l == 0 ? mul0 : mul1);
  const auto& Wskip = m.get(prefix + ".gated_conv.skip_connection.weight", n_skip);
  const auto& Wself = m.get(prefix + ".gated_conv.self_interaction.weight", (int64_t)mul0 * mul0 + (int64_t)mul1 * mul1);
  std::vector<float> ws0((size_t)std::max(in0, 1) * mul0, 0.f), ws1((size_t)std::max(in1, 1) * std::max(mul1, 1), 0.f);
  {
    int64_t o = 0;
    int u0 = 0, u1 = 0;
    for (auto& ib : in_blocks) {
      if (ib.l == 0) {
        for (int u = 0; u < ib.mul; ++u, ++u0)
          for (int w = 0; w < mul0; ++w)
            ws0[(size_t)u0 * mul0 + w] = (float)((double)Wskip[o + (int64_t)u * mul0 + w] / std::sqrt((double)in0) * s_in[ib.ch0 + u]);
        o += (int64_t)ib.mul * mul0;
      } else {
        for (int u = 0; u < ib.mul; ++u, ++u1)
          for (int w = 0; w < mul1; ++w)
            ws1[(size_t)u1 * mul1 + w] = (float)((double)Wskip[o + (int64_t)u * mul1 + w] / std::sqrt((double)in1) * s_in[ib.ch0 + u]);
        o += (int64_t)ib.mul * mul1;
      }
    }
  }
  std::vector<float> wf0((size_t)mul0 * mul0), wf1((size_t)std::max(mul1 * mul1, 1));
  for (int i = 0; i < mul0 * mul0; ++i) wf0[i] = (float)((double)Wself[i] / std::sqrt((double)mul0));
  for (int i = 0; i < mul1 * mul1; ++i) wf1[i] = (float)((double)Wself[(size_t)mul0 * mul0 + i] / std::sqrt((double)mul1));
  // concatenate along K ([self ; skip]) and pack as MFMA B fragments for k_node_update
  auto pack_cat = [](const std::vector<float>& wself, int ks, const std::vector<float>& wskip, int kk, int ncol, int& Kp) {
    Kp = (ks + kk + 7) & ~7;
    const int nt = (ncol + 31) / 32, nsg = Kp / 8;
    std::vector<float4> out((size_t)nt * nsg * 64, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int t = 0; t < nt; ++t)
      for (int sg = 0; sg < nsg; ++sg)
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, c = t * 32 + (lane & 31);
          float v[4] = {0.f, 0.f, 0.f, 0.f};
          for (int st = 0; st < 4; ++st) {
            const int row = 2 * (4 * sg + st) + hh;
            if (c >= ncol) continue;
            if (row < ks) v[st] = wself[(size_t)row * ncol + c];
            else if (row < ks + kk) v[st] = wskip[(size_t)(row - ks) * ncol + c];
          }
          out[((size_t)t * nsg + sg) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
    return out;
  };
  if (wide) {  // k_node_lin_wide: lane (c, hh), element st <-> row 8 g + 4 hh + st (one float4 of a Z row per lane and 4 K-steps)
    auto pack_wide = [](const std::vector<float>& wself, int ks, const std::vector<float>& wskip, int kk, int ncol, int& Kp) {
      Kp = (ks + kk + 7) & ~7;
      const int nt = (ncol + 31) / 32, ng = Kp / 8;
      std::vector<float4> out((size_t)nt * ng * 64, make_float4(0.f, 0.f, 0.f, 0.f));
      for (int t = 0; t < nt; ++t)
        for (int g = 0; g < ng; ++g)
          for (int lane = 0; lane < 64; ++lane) {
            const int hh = lane >> 5, c = t * 32 + (lane & 31);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            for (int st = 0; st < 4; ++st) {
              const int row = 8 * g + 4 * hh + st;
              if (c >= ncol) continue;
              if (row < ks) v[st] = wself[(size_t)row * ncol + c];
              else if (row < ks + kk) v[st] = wskip[(size_t)(row - ks) * ncol + c];
            }
            out[((size_t)t * ng + g) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
          }
      return out;
    };
    L.wn0 = mem.upload(pack_wide(wf0, mul0, ws0, in0, mul0, L.K0w));
    L.wn1 = mem.upload(pack_wide(wf1, mul1, ws1, in1, std::max(mul1, 1), L.K1w));
    return;  // (the compiled-width node-update kernels are not used on the wide path)
  }
  L.wcat0 = mem.upload(pack_cat(wf0, mul0, ws0, in0, mul0, L.K0p));
  L.wcat1 = mem.upload(pack_cat(wf1, mul1, ws1, in1, std::max(mul1, 1), L.K1p));
  // f16x3 node update: the same matrices balanced by exact powers of two — row K (an input channel) times 2^-e_K so that its largest
  // magnitude sits in [0.5, 1), then column w times 2^sW_w so that its largest sits in [2^13, 2^14) — and split hi + lo; K padded to 16.
  // rowf[K] = 2^e_K multiplies the input when the kernel stages it, colf[w] = 2^-sW_w the output column.
  auto pack_cat_h = [&](const std::vector<float>& wself, int ks, const std::vector<float>& wskip, int kk, int ncol, int& Kh,
                        std::vector<float>& rowf, std::vector<float>& colf) {
    Kh = (ks + kk + 15) & ~15;
    auto W = [&](int row, int c) -> double {
      if (c >= ncol) return 0.0;
      if (row < ks) return wself[(size_t)row * ncol + c];
      if (row < ks + kk) return wskip[(size_t)(row - ks) * ncol + c];
      return 0.0;
    };
    rowf.assign(Kh, 1.f);
    std::vector<double> rinv(Kh, 1.0);
    for (int r = 0; r < ks + kk; ++r) {
      double m = 0;
      for (int c = 0; c < ncol; ++c) m = std::max(m, std::fabs(W(r, c)));
      const int ex = pow2_above(m);
      rowf[r] = (float)std::ldexp(1.0, ex);
      rinv[r] = std::ldexp(1.0, -ex);
    }
    const int nt = (ncol + 31) / 32, nst = Kh / 16;
    colf.assign((size_t)nt * 32, 0.f);
    std::vector<double> csc((size_t)nt * 32, 1.0);
    for (int c = 0; c < ncol; ++c) {
      double m = 0;
      for (int r = 0; r < ks + kk; ++r) m = std::max(m, std::fabs(W(r, c) * rinv[r]));
      const int sW = 14 - pow2_above(m);
      csc[c] = std::ldexp(1.0, sW);
      colf[c] = (float)std::ldexp(1.0, -sW);
    }
    std::vector<float4> out((size_t)nt * nst * 2 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int t = 0; t < nt; ++t)
      for (int st = 0; st < nst; ++st)
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, c = t * 32 + (lane & 31);
          double v[8];
          for (int j = 0; j < 8; ++j) {
            const int row = 16 * st + 8 * hh + j;
            v[j] = W(row, c) * rinv[row] * csc[c];
          }
          const size_t b = (((size_t)t * nst + st) * 2) * 64 + lane;
          pack8(v, out[b], out[b + 64]);
        }
    return out;
  };
  {
    std::vector<float> r0, c0, r1, c1;
    L.wh0 = mem.upload(pack_cat_h(wf0, mul0, ws0, in0, mul0, L.K0h, r0, c0));
    L.wh1 = mem.upload(pack_cat_h(wf1, mul1, ws1, in1, std::max(mul1, 1), L.K1h, r1, c1));
    // row factors in the layouts the kernel reads them: activated scalars [mul0], gated vectors [mul1], and the channels of x_in in
    // x_in's own layout (in0 scalars, then in1 vectors x 3 components)
    std::vector<float> ka0(r0.begin(), r0.begin() + mul0), ka1(std::max(mul1, 1), 1.f), kx((size_t)((in0 + 3 * in1 + 3) & ~3), 1.f);
    for (int u = 0; u < mul1; ++u) ka1[u] = r1[u];
    for (int u = 0; u < in0; ++u) kx[u] = r0[mul0 + u];
    for (int u = 0; u < in1; ++u)
      for (int mm = 0; mm < 3; ++mm) kx[in0 + 3 * u + mm] = r1[mul1 + u];
    ka0.resize((size_t)((mul0 + 3) & ~3) + 4, 1.f);
    L.kga0 = mem.upload(ka0); L.kga1 = mem.upload(ka1); L.kgx = mem.upload(kx); L.cg0 = mem.upload(c0); L.cg1 = mem.upload(c1);
  }
}

// SeparableConv block (src/jamun/e3tools/nn/_tensor_product.py:27-47): depth-wise "uvu" instructions in e3nn order — for every
// input block, for sh in (0e, 1e), for l_out = |l1 - l2| .. l1 + l2 kept when it occurs in the output irreps or is 0e — each with
// mul_in weights and its own block of irreps_out_dtp; then o3.Linear(irreps_out_dtp -> G0 x0e + G1 x1e).  Packed in the canonical
// order of jamun_sepconv.hip: weights [A | B | C | D | E], Linear rows scalars [D0 | D3], vectors [D1 | D2 | D4].
LayerDev build_layer_separable(DevArena& mem, const jamun_model& m, const std::string& prefix, const std::vector<InBlock>& in_blocks, const std::vector<double>& s_in,
                               LayerDev& L) {
  const jamun_hparams& hp = m.hp;
  const int mul0 = hp.mul0, mul1 = hp.mul1, G0 = mul0 + mul1, G1 = mul1, H = hp.edge_attr_dim;
  int n0 = 0, n1 = 0;
  for (auto& ib : in_blocks) (ib.l == 0 ? n0 : n1) += ib.mul;
  struct Tri { int kind, u0, mul; int64_t woff, loff; };  // kind: 0 A, 1 B, 2 C, 3 D, 4 E; u0: first canonical channel; offsets: radial_nn.3 row, lin weight
  std::vector<Tri> tri;
  int64_t woff = 0, loff = 0;
  int u0 = 0, u1 = 0;
  for (auto& ib : in_blocks) {
    if (ib.l == 0) {
      tri.push_back({0, u0, ib.mul, woff, loff}); woff += ib.mul; loff += (int64_t)ib.mul * G0;
      tri.push_back({1, u0, ib.mul, woff, loff}); woff += ib.mul; loff += (int64_t)ib.mul * G1;
      u0 += ib.mul;
    } else {
      tri.push_back({2, u1, ib.mul, woff, loff}); woff += ib.mul; loff += (int64_t)ib.mul * G1;
      tri.push_back({3, u1, ib.mul, woff, loff}); woff += ib.mul; loff += (int64_t)ib.mul * G0;
      tri.push_back({4, u1, ib.mul, woff, loff}); woff += ib.mul; loff += (int64_t)ib.mul * G1;
      u1 += ib.mul;
    }
  }
  const auto& W3 = m.get(prefix + ".gated_conv.f.f.radial_nn.3.weight", woff * H);
  const auto& b3 = m.get(prefix + ".gated_conv.f.f.radial_nn.3.bias", woff);
  const auto& WL = m.get(prefix + ".gated_conv.f.f.tp.lin.weight", loff);
  // input noise scaling per canonical channel
  std::vector<double> s0(n0, 1.0), s1(n1, 1.0);
  {
    int a0 = 0, a1 = 0;
    for (auto& ib : in_blocks)
      for (int u = 0; u < ib.mul; ++u) (ib.l == 0 ? s0[a0++] : s1[a1++]) = s_in[ib.ch0 + u];
  }
  const int NW = 2 * n0 + 3 * n1, NWp = (NW + 31) & ~31, n_ct = NWp / 32;
  const int base[5] = {0, n0, 2 * n0, 2 * n0 + n1, 2 * n0 + 2 * n1};
  // path weight sqrt(2 l_out + 1) x Clebsch-Gordan factor x the sqrt(3) of Y_1 = sqrt(3) v:  A 1, B sqrt(3) (delta/sqrt(3) sqrt(3) sqrt(3)),
  // C 1 (sqrt(3) delta/sqrt(3)), D 1 (delta/sqrt(3) sqrt(3)), E sign sqrt(3) (eps/sqrt(6)) sqrt(3) = sign sqrt(3/2)
  const double fac[5] = {1.0, std::sqrt(3.0), 1.0, 1.0, (double)hp.w3j_111_sign * std::sqrt(1.5)};
  std::vector<double> w2c((size_t)(H + 1) * NWp, 0.0);
  for (const Tri& t : tri)
    for (int u = 0; u < t.mul; ++u) {
      const double sc = fac[t.kind] * (t.kind < 2 ? s0[t.u0 + u] : s1[t.u0 + u]);
      const int col = base[t.kind] + t.u0 + u;
      for (int k = 0; k <= H; ++k)
        w2c[(size_t)k * NWp + col] = sc * (k < H ? (double)W3[(size_t)(t.woff + u) * H + k] : (double)b3[t.woff + u]);
    }
  // B fragments of the f16x3 weight GEMM of k_sep_fused: column tiles A 0..3 (x0 -> 0e, channel u at column 32 ct + c), B 4..7, C 8, D 9,
  // E 10; every column balanced by its own power of two (the depth-wise weights inherit the spread of the channels they multiply),
  // split hi + lo; the bias row (hidden unit H: the radial MLP's output bias) is added in fp32 after the product
  // (the envelope of k_sep_fused / k_sep_linear, with the reason: the same texts as sep_conv_unsupported, which sees the edge stride too)
  if (n0 > 128 || n1 > 32) throw Err(JAMUN_ERR_INVALID, "SeparableConv: input irreps wider than 128x0e + 32x1e");
  if (H != 64) throw Err(JAMUN_ERR_INVALID, "SeparableConv: radial MLP with other than 64 hidden units");
  (void)n_ct;
  std::vector<float> cfw(352, 0.f), bias(352, 0.f);
  std::vector<float4> w2b((size_t)4 * 11 * 2 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
  {
    auto old_col = [&](int nc) -> int {  // new column -> canonical column of w2c (-1: padding)
      if (nc < 128) return nc < n0 ? base[0] + nc : -1;
      if (nc < 256) return nc - 128 < n0 ? base[1] + (nc - 128) : -1;
      const int kind = 2 + (nc - 256) / 32, u = (nc - 256) % 32;
      return u < n1 ? base[kind] + u : -1;
    };
    std::vector<double> csc(352, 1.0);
    for (int nc = 0; nc < 352; ++nc) {
      const int oc = old_col(nc);
      if (oc < 0) continue;
      double mx = 0;
      for (int k = 0; k < H; ++k) mx = std::max(mx, std::fabs(w2c[(size_t)k * NWp + oc]));
      int ex = 0;
      if (mx > 0 && std::isfinite(mx)) std::frexp(mx, &ex);
      const int sW = 14 - std::max(-40, std::min(40, ex));
      csc[nc] = std::ldexp(1.0, sW);
      cfw[nc] = (float)std::ldexp(1.0, -sW);
      bias[nc] = (float)w2c[(size_t)H * NWp + oc];
    }
    for (int s4 = 0; s4 < 4; ++s4)
      for (int ct = 0; ct < 11; ++ct)
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, nc = 32 * ct + (lane & 31), oc = old_col(nc);
          uint32_t hw[4], lw[4];
          for (int i = 0; i < 4; ++i) {
            uint16_t hp[2], lp[2];
            for (int e = 0; e < 2; ++e) {
              const int k = 16 * s4 + 8 * hh + 2 * i + e;
              split_f16(oc >= 0 ? w2c[(size_t)k * NWp + oc] * csc[nc] : 0.0, hp[e], lp[e]);
            }
            hw[i] = (uint32_t)hp[0] | ((uint32_t)hp[1] << 16);
            lw[i] = (uint32_t)lp[0] | ((uint32_t)lp[1] << 16);
          }
          const size_t bidx = (((size_t)s4 * 11 + ct) * 2) * 64 + lane;
          std::memcpy(&w2b[bidx], hw, 16);
          std::memcpy(&w2b[bidx + 64], lw, 16);
        }
  }
  const int K0 = n0 + n1, K1 = n0 + 2 * n1;
  std::vector<float> wl0((size_t)K0 * G0, 0.f), wl1((size_t)std::max(K1 * G1, 1), 0.f);
  for (const Tri& t : tri)
    for (int u = 0; u < t.mul; ++u) {
      const bool scalar_out = t.kind == 0 || t.kind == 3;
      const int G = scalar_out ? G0 : G1;
      const int row = t.kind == 0 ? t.u0 + u : t.kind == 3 ? n0 + t.u0 + u : t.kind == 1 ? t.u0 + u : t.kind == 2 ? n0 + t.u0 + u : n0 + n1 + t.u0 + u;
      const double nrm = 1.0 / std::sqrt((double)(scalar_out ? K0 : K1));
      for (int w = 0; w < G; ++w) (scalar_out ? wl0 : wl1)[(size_t)row * G + w] = (float)((double)WL[t.loff + (int64_t)u * G + w] * nrm);
    }
  L.sep.w2b = mem.upload(w2b); L.sep.cfw = mem.upload(cfw); L.sep.bias = mem.upload(bias); L.sep.wl0 = mem.upload(wl0); L.sep.wl1 = mem.upload(wl1);
  L.sep.n0 = n0; L.sep.n1 = n1;
  L.p0.nt = (G0 + 31) / 32;  // (the node update reads the slab widths from here)
  L.p1.nt = (G1 + 31) / 32;
  L.p0.planes = 1; L.p1.planes = 3;
  L.in0 = n0; L.in1 = n1; L.XSin = n0 + 3 * n1;
  L.tp_numel = woff;
  build_layer_common(mem, m, prefix, in_blocks, s_in, L, n0, n1);
  {  // static scale of h~ (bounded by the radial MLP's first layer: build_layer_common)
    int ex = 0;
    std::frexp(0.5 * (double)L.dg.hmax2, &ex);
    L.sep.sH = std::max(-40, std::min(40, 14 - ex));
  }
  return L;
}

}  // namespace

LayerDev build_layer(DevArena& mem, DevArena& dg_mem, const jamun_model& m, const std::string& prefix, const std::vector<InBlock>& in_blocks,
                     const std::vector<double>& s_in, int n_slices,
                     const std::vector<float>* uniq_rows, int row_len, bool pack_dg, const std::vector<float>* all_rows, bool wide) {
  const jamun_hparams& hp = m.hp;
  const int mul0 = hp.mul0, mul1 = hp.mul1, G0 = mul0 + mul1, G1 = mul1, H = hp.edge_attr_dim;
  LayerDev L;
  // ---- FullyConnectedTensorProduct instruction table (e3nn order: for i1, for i2 in (0e,1e), for i_out in (0e,1e))
  struct Ins { int b, l2, lo; int64_t off; };
  std::vector<Ins> ins;
  int64_t off = 0;
  double sum0 = 0, sum1 = 0;  // sum over instructions of mul1*mul2 feeding each output irrep
  for (size_t b = 0; b < in_blocks.size(); ++b)
    for (int l2 = 0; l2 <= 1; ++l2)
      for (int lo = 0; lo <= 1; ++lo) {
        const int l1 = in_blocks[b].l;
        if (lo < std::abs(l1 - l2) || lo > l1 + l2) continue;
        const int gout = lo == 0 ? G0 : G1;
        if (gout == 0) continue;
        ins.push_back({(int)b, l2, lo, off});
        off += (int64_t)in_blocks[b].mul * gout;
        (lo == 0 ? sum0 : sum1) += in_blocks[b].mul;
      }
  L.tp_numel = off;
  if (hp.separable) return build_layer_separable(mem, m, prefix, in_blocks, s_in, L);
  const auto& W3 = m.get(prefix + ".gated_conv.f.f.radial_nn.3.weight", off * H);
  const auto& b3 = m.get(prefix + ".gated_conv.f.f.radial_nn.3.bias", off);
  const double c0 = std::sqrt(1.0 / sum0), c1 = sum1 > 0 ? std::sqrt(3.0 / sum1) : 0.0;
  auto find = [&](int b, int l2, int lo) -> int64_t {
    for (auto& i : ins)
      if (i.b == b && i.l2 == l2 && i.lo == lo) return i.off;
    throw Err(JAMUN_ERR_INVALID, "internal: missing tensor-product instruction");
  };
  std::vector<UEntry> x0e, dote, x0ve, x1e, crosse;
  int in0 = 0, in1 = 0;
  for (size_t b = 0; b < in_blocks.size(); ++b) {
    const InBlock& ib = in_blocks[b];
    for (int u = 0; u < ib.mul; ++u) {
      const double s = s_in[ib.ch0 + u];
      if (ib.l == 0) {
        x0e.push_back({JAMUN_T_X0, 0, ib.xoff + u, find(b, 0, 0) + (int64_t)u * G0, c0 * s});
        if (G1) x0ve.push_back({JAMUN_T_X0V, 0, ib.xoff + u, find(b, 1, 1) + (int64_t)u * G1, c1 * s});
      } else {
        dote.push_back({JAMUN_T_DOT, 0, ib.xoff + 3 * u, find(b, 1, 0) + (int64_t)u * G0, c0 * s});
        x1e.push_back({JAMUN_T_X1C, 0, ib.xoff + 3 * u, find(b, 0, 1) + (int64_t)u * G1, c1 / std::sqrt(3.0) * s});
        crosse.push_back({JAMUN_T_X1C, 1, ib.xoff + 3 * u, find(b, 1, 1) + (int64_t)u * G1,
                          c1 * (double)hp.w3j_111_sign / std::sqrt(2.0) * s});
      }
    }
    if (ib.l == 0) in0 += ib.mul; else in1 += ib.mul;
  }
  L.in0 = in0; L.in1 = in1; L.XSin = in0 + 3 * in1;
  auto chunked = [](const std::vector<UEntry>& v, int type, std::vector<UBlock>& out) {
    for (size_t i = 0; i < v.size(); i += 64) {
      UBlock b; b.type = type;
      b.e.assign(v.begin() + i, v.begin() + std::min(v.size(), i + 64));
      pad_even(b);
      out.push_back(b);
    }
  };
  std::vector<UBlock> blocks0, blocks1;
  chunked(x0e, JAMUN_T_X0, blocks0);
  chunked(dote, JAMUN_T_DOT, blocks0);
  chunked(x0ve, JAMUN_T_X0V, blocks1);
  for (size_t i = 0; i < x1e.size(); i += 32) {
    UBlock b; b.type = JAMUN_T_X1C;
    const size_t hi = std::min(x1e.size(), i + 32);
    b.e.assign(x1e.begin() + i, x1e.begin() + hi);
    b.e.insert(b.e.end(), crosse.begin() + i, crosse.begin() + hi);
    pad_even(b);
    blocks1.push_back(b);
  }
  if (wide) {  // the wide path (jamun_wide.hip): k_conv_wide's chunking, no specialised kernels
    L.p0 = pack_problem(mem, blocks0, 1, G0, n_slices, JAMUN_WIDE_KSUB0, W3, b3, H, true);
    L.p1 = pack_problem(mem, blocks1, 3, G1, n_slices, JAMUN_WIDE_KSUB1, W3, b3, H, true);
    build_layer_common(mem, m, prefix, in_blocks, s_in, L, in0, in1, true);
    return L;
  }
  L.p0 = pack_problem(mem, blocks0, 1, G0, n_slices, JAMUN_KSUB0, W3, b3, H);
  L.p1 = pack_problem(mem, blocks1, 3, G1, n_slices, JAMUN_KSUB1, W3, b3, H);

  bool x0_contig = true;
  for (size_t i = 1; i < x0ve.size(); ++i) x0_contig = x0_contig && x0ve[i].xoff == x0ve[0].xoff + (int)i;
  const int NT0 = (G0 + 31) / 32;

  // ---- destination-grouped VALU-forming kernel (jamun_conv_dg.hip): weights as 64-lane float4 blocks in MFMA operand order
  if (pack_dg && mul0 == 120 && mul1 == 32 && x0e.size() == 120 && dote.size() == 32 && x1e.size() == 32 && crosse.size() == 32 &&
      x0ve.size() == 120 && x0_contig && x0e[0].xoff == 0 && dote[0].xoff == 120) {
    const int n_k = H + 1;
    auto Wk = [&](int k, int64_t p) -> double { return (k < H) ? (double)W3[(size_t)p * H + k] : (double)b3[p]; };
    std::vector<float4> wx((size_t)n_k * 5 * 16 * 64), wd((size_t)n_k * 5 * 4 * 64), wv((size_t)n_k * 2 * 4 * 64), wt((size_t)n_k * 15 * 64);
    for (int k = 0; k < n_k; ++k) {
      for (int t = 0; t < 5; ++t)
        for (int g = 0; g < 16; ++g)
          for (int lane = 0; lane < 64; ++lane) {
            const int hh = lane >> 5, c = lane & 31, col = 32 * t + c;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            for (int st = 0; st < 4; ++st) {
              const int u = 8 * g + 4 * hh + st;
              if (u < 120 && col < G0) v[st] = (float)(Wk(k, x0e[u].wbase + col) * x0e[u].scale);
            }
            wx[(((size_t)k * 5 + t) * 16 + g) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
            if (g < 4) {
              float d[4] = {0.f, 0.f, 0.f, 0.f};
              for (int st = 0; st < 4; ++st) {
                const int u = 8 * g + 4 * hh + st;
                if (col < G0) d[st] = (float)(Wk(k, dote[u].wbase + col) * dote[u].scale);
              }
              wd[(((size_t)k * 5 + t) * 4 + g) * 64 + lane] = make_float4(d[0], d[1], d[2], d[3]);
            }
          }
      for (int lane = 0; lane < 64; ++lane) {
        const int kq = lane >> 4, c = lane & 15;
        for (int ch = 0; ch < 2; ++ch) {
          const int col = 16 * ch + c;
          for (int g = 0; g < 4; ++g) {  // vector planes: kappa = 16 g + 4 kq + st over [x1 (32) | cross (32)]
            float v[4];
            for (int st = 0; st < 4; ++st) {
              const int kap = 16 * g + 4 * kq + st;
              const UEntry& e = kap < 32 ? x1e[kap] : crosse[kap - 32];
              v[st] = (float)(Wk(k, e.wbase + col) * e.scale);
            }
            wv[(((size_t)k * 2 + ch) * 4 + g) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
          }
        }
      }
      for (int g = 0; g < 15; ++g)  // T pre-pass (k_tprod, 32x32x2): lane (c = w', hh), u = 8 g + 4 hh + st over the 120 scalar inputs
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, c = lane & 31;
          float v[4];
          for (int st = 0; st < 4; ++st) {
            const int u = 8 * g + 4 * hh + st;
            v[st] = (float)(Wk(k, x0ve[u].wbase + c) * x0ve[u].scale);
          }
          wt[((size_t)k * 15 + g) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    L.dg.wx = dg_mem.upload(wx); L.dg.wd = dg_mem.upload(wd); L.dg.wv = dg_mem.upload(wv); L.dg.wt = dg_mem.upload(wt);
    // f16x3 contraction: the same weights BALANCED by exact powers of two and split into hi + lo halves.  An f16 pair carries 22 bits
    // only while its lo half is a normal number, i.e. within 2^-14 .. 2^-17 of the largest value sharing its scale, and trained
    // checkpoints spread their channels over many octaves (a feature channel that is small has large weights, and the other way
    // round), so one scale per tensor is not enough:
    //   * input channel u: its weight rows (k, u) times 2^-e_u (largest magnitude over k and columns -> [0.5, 1)); the kernels multiply
    //     the feature rows by 2^e_u when they stage them (DgDev::gx, in the layout of a feature row), BEFORE they measure the maxima their
    //     dynamic scales come from — every input then enters with the weight of its contribution.  The vector channel u shares one
    //     exponent over its three blocks (dot, x1, cross); the T pre-pass has its own (gT);
    //   * output column w: times 2^sB_w (largest -> [2^13, 2^14)); undone per column in the kernels' epilogues (cf0 / cf1 / cfT).
    // one block = 64 lanes x 8 halves = the B fragment of one v_mfma_f32_32x32x16_f16 (lane (c, hh): inputs 16 g + 8 hh + j,
    // column 32 t + c) or v_mfma_f32_16x16x32_f16 (lane (c16, kq): kappa = 32 G + 8 kq + j, column 16 ch + c16)
    {
      auto row_exp = [&](const UEntry& e, int ncols) {
        double m = 0;
        for (int k = 0; k < n_k; ++k) for (int col = 0; col < ncols; ++col) m = std::max(m, std::fabs(Wk(k, e.wbase + col) * e.scale));
        return m;
      };
      std::vector<int> e0(120), e1(32), eT(120);
      for (int u = 0; u < 120; ++u) { e0[u] = pow2_above(row_exp(x0e[u], G0)); eT[u] = pow2_above(row_exp(x0ve[u], G1)); }
      for (int u = 0; u < 32; ++u) e1[u] = pow2_above(std::max(row_exp(dote[u], G0), std::max(row_exp(x1e[u], G1), row_exp(crosse[u], G1))));
      auto Wg = [&](const UEntry& e, int ex, int k, int col) { return std::ldexp(Wk(k, e.wbase + col) * e.scale, -ex); };
      std::vector<double> sc0(160, 1.0), sc1(32, 1.0), scT(32, 1.0);  // column scales 2^sB_w
      std::vector<float> cf0(160, 0.f), cf1(32, 0.f), cfT(32, 0.f);   // ... and their inverses for the epilogues
      for (int col = 0; col < G0; ++col) {
        double m = 0;
        for (int k = 0; k < n_k; ++k) {
          for (int u = 0; u < 120; ++u) m = std::max(m, std::fabs(Wg(x0e[u], e0[u], k, col)));
          for (int u = 0; u < 32; ++u) m = std::max(m, std::fabs(Wg(dote[u], e1[u], k, col)));
        }
        const int sB = 14 - pow2_above(m);
        sc0[col] = std::ldexp(1.0, sB); cf0[col] = (float)std::ldexp(1.0, -sB);
      }
      for (int col = 0; col < G1; ++col) {
        double m = 0, mt = 0;
        for (int k = 0; k < n_k; ++k) {
          for (int u = 0; u < 32; ++u) m = std::max(m, std::max(std::fabs(Wg(x1e[u], e1[u], k, col)), std::fabs(Wg(crosse[u], e1[u], k, col))));
          for (int u = 0; u < 120; ++u) mt = std::max(mt, std::fabs(Wg(x0ve[u], eT[u], k, col)));
        }
        const int sB = 14 - pow2_above(m), sT = 14 - pow2_above(mt);
        sc1[col] = std::ldexp(1.0, sB); cf1[col] = (float)std::ldexp(1.0, -sB);
        scT[col] = std::ldexp(1.0, sT); cfT[col] = (float)std::ldexp(1.0, -sT);
      }
      {
        std::vector<float> gx(216), gT(128, 1.f);
        for (int u = 0; u < 120; ++u) { gx[u] = (float)std::ldexp(1.0, e0[u]); gT[u] = (float)std::ldexp(1.0, eT[u]); }
        for (int u = 0; u < 32; ++u) for (int mm = 0; mm < 3; ++mm) gx[120 + 3 * u + mm] = (float)std::ldexp(1.0, e1[u]);
        L.dg.gx = dg_mem.upload(gx); L.dg.gT = dg_mem.upload(gT);
        L.dg.cf0 = dg_mem.upload(cf0); L.dg.cf1 = dg_mem.upload(cf1); L.dg.cfT = dg_mem.upload(cfT);
      }
      L.dg.sB = 0;  // (the column factors carry the weight scales)
      std::vector<float4> wxh((size_t)n_k * 5 * 8 * 2 * 64), wdh((size_t)n_k * 5 * 2 * 2 * 64), wvh((size_t)n_k * 2 * 2 * 2 * 64);
      for (int k = 0; k < n_k; ++k) {
        for (int t = 0; t < 5; ++t)
          for (int lane = 0; lane < 64; ++lane) {
            const int hh = lane >> 5, c = lane & 31, col = 32 * t + c;
            for (int g = 0; g < 8; ++g) {
              double v[8];
              for (int j = 0; j < 8; ++j) {
                const int u = 16 * g + 8 * hh + j;
                v[j] = (u < 120 && col < G0) ? Wg(x0e[u], e0[u], k, col) * sc0[col] : 0.0;
              }
              const size_t b = ((((size_t)k * 5 + t) * 8 + g) * 2) * 64 + lane;
              pack8(v, wxh[b], wxh[b + 64]);
            }
            for (int g = 0; g < 2; ++g) {
              double v[8];
              for (int j = 0; j < 8; ++j) {
                const int u = 16 * g + 8 * hh + j;
                v[j] = col < G0 ? Wg(dote[u], e1[u], k, col) * sc0[col] : 0.0;
              }
              const size_t b = ((((size_t)k * 5 + t) * 2 + g) * 2) * 64 + lane;
              pack8(v, wdh[b], wdh[b + 64]);
            }
          }
        for (int ch = 0; ch < 2; ++ch)
          for (int G = 0; G < 2; ++G)
            for (int lane = 0; lane < 64; ++lane) {
              const int kq = lane >> 4, c = lane & 15, col = 16 * ch + c;
              double v[8];
              for (int j = 0; j < 8; ++j) {
                const int kap = 32 * G + 8 * kq + j;  // input order of the vector planes' A tiles: 2 u + {x1, cross}
                const UEntry& e = (kap & 1) ? crosse[kap >> 1] : x1e[kap >> 1];
                v[j] = Wg(e, e1[kap >> 1], k, col) * sc1[col];
              }
              const size_t b = ((((size_t)k * 2 + ch) * 2 + G) * 2) * 64 + lane;
              pack8(v, wvh[b], wvh[b + 64]);
            }
      }
      // one stream per (hidden unit, matrix wave) in the order the wave consumes it — 34 blocks: four chunks of the scalar inputs
      // (own tile: groups 2c, 2c+1 as hi, lo, hi, lo; then the wave's group of scalar tile 4, w + 4 (c >> 1), when it falls into this
      // chunk — (c & 1) == (w >> 1) — else unused), the dot inputs (own tile groups 0, 1; tile 4: group w for w < 2), the vector
      // planes (column half w >> 1: groups 0, 1): every load is (uniform base of (k, w)) + constant + lane
      std::vector<float4> wh((size_t)n_k * 4 * 34 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
      auto copy_blocks = [&](const std::vector<float4>& src, size_t src_block, size_t dst_block) {  // hi and lo block
        std::copy(src.begin() + src_block * 64, src.begin() + (src_block + 2) * 64, wh.begin() + dst_block * 64);
      };
      for (int k = 0; k < n_k; ++k)
        for (int w = 0; w < 4; ++w) {
          const size_t base = ((size_t)k * 4 + w) * 34;
          for (int c = 0; c < 4; ++c) {
            for (int gi = 0; gi < 2; ++gi) copy_blocks(wxh, (((size_t)k * 5 + w) * 8 + 2 * c + gi) * 2, base + 6 * c + 2 * gi);
            if ((w >> 1) == (c & 1)) copy_blocks(wxh, (((size_t)k * 5 + 4) * 8 + w + 4 * (c >> 1)) * 2, base + 6 * c + 4);
          }
          for (int g = 0; g < 2; ++g) copy_blocks(wdh, (((size_t)k * 5 + w) * 2 + g) * 2, base + 24 + 2 * g);
          if (w < 2) copy_blocks(wdh, (((size_t)k * 5 + 4) * 2 + w) * 2, base + 28);
          for (int G = 0; G < 2; ++G) copy_blocks(wvh, (((size_t)k * 2 + (w >> 1)) * 2 + G) * 2, base + 30 + 2 * G);
        }
      L.dg.wxh = dg_mem.upload(wh);
      // T pre-pass (k_tprod_h): scalar inputs -> vector rows, weights as the A operand of v_mfma_f32_32x32x16_f16
      {
        L.dg.sBt = 0;  // (balanced per input channel (gT) and per column (cfT), as the contraction's weights)
        std::vector<float4> wth((size_t)n_k * 16 * 64);
        for (int k = 0; k < n_k; ++k)
          for (int g = 0; g < 8; ++g)
            for (int lane = 0; lane < 64; ++lane) {
              const int hh = lane >> 5, c = lane & 31;
              double v[8];
              for (int j = 0; j < 8; ++j) {
                const int u = 16 * g + 8 * hh + j;
                v[j] = (u < 120 && c < G1) ? Wg(x0ve[u], eT[u], k, c) * scT[c] : 0.0;
              }
              const size_t b = ((size_t)k * 16 + 2 * g) * 64 + lane;
              pack8(v, wth[b], wth[b + 64]);
            }
        L.dg.wth = dg_mem.upload(wth);
      }
      // jamun_conv_mf.hip: the A operand of the contraction is the ACCUMULATOR of the forming MFMA (lane = destination, registers =
      // channels), so half p of lane (column c, hh) in K-step s2 is input u = 16 s2 + (p & 3) + 8 (p >> 2) + 4 hh of the wave's 32
      // channels.  Same scale 2^sB as the stream of k_conv_dg.  sTw: 2^sTw x (largest column sum of the T weights) < 1, so that
      // T_k = x0 W times 2^(sX + sTw) stays below 2^14 with |x| 2^sX < 2^14.
      {
        double wcs = 0;
        for (int k = 0; k < n_k; ++k)
          for (int c = 0; c < G1; ++c) {
            double cs = 0;
            for (int u = 0; u < 120; ++u) cs += std::fabs(Wg(x0ve[u], e0[u], k, c));  // (the gauge of the conv kernel's scalar channels: |T| <= max|x'| x this)
            wcs = std::max(wcs, cs);
          }
        int exs = 0;
        if (wcs > 0 && std::isfinite(wcs)) std::frexp(wcs, &exs);
        L.dg.sTw = std::max(-40, std::min(40, -exs));
        auto u_of = [](int s2, int hh, int p) { return 16 * s2 + (p & 3) + 8 * (p >> 2) + 4 * hh; };
        // stream of hidden unit k: 124 blocks = waves 0..3 (scalar channels 32 w ..: 20 blocks, (hi, lo) per (output tile n, K-step s2)),
        // wave 4 (dot inputs: 20), waves 5..7 (vector plane: x1 inputs 4 blocks, cross inputs 4 — the same for every plane)
        std::vector<float4> wm((size_t)n_k * 124 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
        for (int k = 0; k < n_k; ++k) {
          const size_t kb = (size_t)k * 124 * 64;
          for (int lane = 0; lane < 64; ++lane) {
            const int hh = lane >> 5, c = lane & 31;
            for (int w = 0; w < 5; ++w)
              for (int n = 0; n < 5; ++n)
                for (int s2 = 0; s2 < 2; ++s2) {
                  const int col = 32 * n + c;
                  double v[8];
                  for (int p = 0; p < 8; ++p) {
                    const int u = 32 * w + u_of(s2, hh, p);
                    if (w < 4) v[p] = (u < 120 && col < G0) ? Wg(x0e[u], e0[u], k, col) * sc0[col] : 0.0;
                    else v[p] = col < G0 ? Wg(dote[u - 128], e1[u - 128], k, col) * sc0[col] : 0.0;
                  }
                  const size_t b = kb + (size_t)(20 * w + 2 * (2 * n + s2)) * 64 + lane;
                  pack8(v, wm[b], wm[b + 64]);
                }
            for (int m = 0; m < 3; ++m)
              for (int part = 0; part < 2; ++part)  // x1 inputs, then cross inputs -> vector rows (32 columns)
                for (int s2 = 0; s2 < 2; ++s2) {
                  double v[8];
                  for (int p = 0; p < 8; ++p) {
                    const UEntry& e = part == 0 ? x1e[u_of(s2, hh, p)] : crosse[u_of(s2, hh, p)];
                    v[p] = c < G1 ? Wg(e, e1[u_of(s2, hh, p)], k, c) * sc1[c] : 0.0;
                  }
                  const size_t b = kb + (size_t)(100 + 8 * m + 4 * part + 2 * s2) * 64 + lane;
                  pack8(v, wm[b], wm[b + 64]);
                }
          }
        }
        L.dg.wm = dg_mem.upload(wm);
        // tail tiles (k_tail_contract): the vector outputs take x1, cross AND the scalar channels times v_m (no T pre-pass there) in one
        // accumulator, so the three weight blocks share one column scale; 24 blocks per hidden unit: x1 (2 K-steps x hi, lo), cross,
        // then the scalar channel tiles w = 0..3 (input gauge e0: the rows are staged once, with the conv kernel's channel factors)
        {
          std::vector<double> sct(32, 1.0);
          std::vector<float> cf1t(32, 0.f);
          for (int col = 0; col < G1; ++col) {
            double mx = 0;
            for (int k = 0; k < n_k; ++k) {
              for (int u = 0; u < 32; ++u) mx = std::max(mx, std::max(std::fabs(Wg(x1e[u], e1[u], k, col)), std::fabs(Wg(crosse[u], e1[u], k, col))));
              for (int u = 0; u < 120; ++u) mx = std::max(mx, std::fabs(Wg(x0ve[u], e0[u], k, col)));
            }
            const int sB = 14 - pow2_above(mx);
            sct[col] = std::ldexp(1.0, sB); cf1t[col] = (float)std::ldexp(1.0, -sB);
          }
          std::vector<float4> wmt((size_t)n_k * 24 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
          for (int k = 0; k < n_k; ++k)
            for (int lane = 0; lane < 64; ++lane) {
              const int hh = lane >> 5, c = lane & 31;
              for (int g = 0; g < 6; ++g)
                for (int s2 = 0; s2 < 2; ++s2) {
                  double v[8];
                  for (int pp = 0; pp < 8; ++pp) {
                    const int ul = u_of(s2, hh, pp);
                    if (c >= G1) v[pp] = 0.0;
                    else if (g == 0) v[pp] = Wg(x1e[ul], e1[ul], k, c) * sct[c];
                    else if (g == 1) v[pp] = Wg(crosse[ul], e1[ul], k, c) * sct[c];
                    else { const int u = 32 * (g - 2) + ul; v[pp] = u < 120 ? Wg(x0ve[u], e0[u], k, c) * sct[c] : 0.0; }
                  }
                  const size_t b = ((size_t)k * 24 + 4 * g + 2 * s2) * 64 + lane;
                  pack8(v, wmt[b], wmt[b + 64]);
                }
            }
          L.dg.wmt = dg_mem.upload(wmt);
          L.dg.cf1t = dg_mem.upload(cf1t);
        }
      }
    }
  }

  // ---- initial projector: input-times-weight table (inputs are constant per distinct embedding row) for k_conv_init_v and k_conv_mfi
  if (uniq_rows && G0 <= 32 * NT0 && G1 <= 32) {
    bool scalar_only = true;
    for (auto& ib : in_blocks) scalar_only = scalar_only && ib.l == 0;
    const int U = (int)(uniq_rows->size() / (size_t)row_len);
    const int tt_row = 32 * (NT0 + 1);
    if (scalar_only && U > 0 && (size_t)U * tt_row * (H + 1) * sizeof(float) <= ((size_t)256 << 20)) {
      std::vector<float> tt((size_t)(H + 1) * U * tt_row, 0.f);
      for (int k = 0; k <= H; ++k)
        for (int uid = 0; uid < U; ++uid) {
          const float* xr = uniq_rows->data() + (size_t)uid * row_len;
          float* out = tt.data() + ((size_t)k * U + uid) * tt_row;
          for (int w = 0; w < G0; ++w) {
            double acc = 0;
            for (const UEntry& e : x0e) {
              const int64_t p = e.wbase + w;
              acc += (double)xr[e.xoff] * ((k < H) ? (double)W3[(size_t)p * H + k] : (double)b3[p]) * e.scale;
            }
            out[w] = (float)acc;
          }
          for (int w = 0; w < G1; ++w) {
            double acc = 0;
            for (const UEntry& e : x0ve) {
              const int64_t p = e.wbase + w;
              acc += (double)xr[e.xoff] * ((k < H) ? (double)W3[(size_t)p * H + k] : (double)b3[p]) * e.scale;
            }
            out[32 * NT0 + w] = (float)acc;
          }
        }
      L.tt_U = U;
      if (NT0 == 5 && G0 <= 152 && G1 <= 32) {  // scalar columns 0..127 as they are, then per lane u (column 128+u, vector column u)
        std::vector<float> tt2((size_t)(H + 1) * U * 192, 0.f);
        for (int k = 0; k <= H; ++k)
          for (int uid = 0; uid < U; ++uid) {
            const float* in = tt.data() + ((size_t)k * U + uid) * tt_row;
            float* out = tt2.data() + ((size_t)k * U + uid) * 192;
            for (int c = 0; c < 128; ++c) out[c] = in[c];
            for (int u = 0; u < 32; ++u) {
              out[128 + 2 * u] = u < 24 ? in[128 + u] : 0.f;
              out[128 + 2 * u + 1] = in[32 * NT0 + u];
            }
          }
        L.tt2 = mem.upload(tt2);
      }
      if (NT0 == 5 && G0 <= 160 && G1 <= 32 && U <= 128) {
        const int UT = U <= 32 ? 1 : (U <= 64 ? 2 : 4);
        L.tab_ut = UT;
        // k_conv_mfi: blocks 4 r + 2 s2 + {hi, lo}; half p of lane (column c, hh) <-> uid 16 s2 + (p & 3) + 8 (p >> 2) + 4 hh (the
        // accumulator layout of the forming MFMA); r < 5: scalar-output columns 32 r + c, r = 5: the vector columns
        double tmax = 0;
        for (float v : tt) tmax = std::max(tmax, (double)std::fabs(v));
        int ex = 0;
        if (tmax > 0 && std::isfinite(tmax)) std::frexp(tmax, &ex);
        L.tab_sB = std::max(-40, std::min(40, 14 - ex));
        const double sc = std::ldexp(1.0, L.tab_sB);
        std::vector<float4> tw((size_t)(H + 1) * 6 * 4 * UT * 64, make_float4(0.f, 0.f, 0.f, 0.f));
        for (int k = 0; k <= H; ++k)
          for (int r = 0; r < 6; ++r)
            for (int ts = 0; ts < 2 * UT; ++ts)
              for (int lane = 0; lane < 64; ++lane) {
                const int s2 = ts & 1, ut = ts >> 1;
                const int hh = lane >> 5, c = lane & 31;
                const int col = r < 5 ? 32 * r + c : 32 * NT0 + c;
                const bool col_ok = r < 5 ? col < G0 : c < G1;
                double v[8];
                for (int pp = 0; pp < 8; ++pp) {
                  const int uid = 32 * ut + 16 * s2 + (pp & 3) + 8 * (pp >> 2) + 4 * hh;
                  v[pp] = ((col_ok && uid < U) ? (double)tt[((size_t)k * U + uid) * tt_row + col] : 0.0) * sc;
                }
                const size_t b = (((size_t)k * 6 + r) * 4 * UT + 4 * ut + 2 * s2) * 64 + lane;
                pack8(v, tw[b], tw[b + 64]);
              }
        L.tabw = mem.upload(tw);
      }
    }
  }

  // ---- k_conv_mfx: the initial projector formed from the feature rows themselves (scalar inputs only, at most 64 channels): weights
  // balanced per input channel (2^-e_u; the factor goes into the stored rows) and per output column (2^sB_w, undone by xcf0 / xcf1), the
  // rows x 2^e_u x 2^x_sX (ONE static scale: the rows are constants of (topology, sigma)) split hi + lo on the host, two atoms per word
  if (all_rows && row_len > 0 && row_len <= 64 && in1 == 0 && NT0 == 5 && G1 <= 32 && G1 > 0 && (int)x0e.size() == row_len && (int)x0ve.size() == row_len) {
    const int n_k = H + 1, C = row_len;
    auto Wk = [&](int k, int64_t p) -> double { return (k < H) ? (double)W3[(size_t)p * H + k] : (double)b3[p]; };
    std::vector<const UEntry*> es(64, nullptr), ev(64, nullptr);  // by feature column (xoff)
    for (const UEntry& e : x0e) es[e.xoff] = &e;
    for (const UEntry& e : x0ve) ev[e.xoff] = &e;
    std::vector<int> eu(64, 0);
    for (int u = 0; u < C; ++u) {
      double mx = 0;
      for (int k = 0; k < n_k; ++k) {
        for (int col = 0; col < G0; ++col) mx = std::max(mx, std::fabs(Wk(k, es[u]->wbase + col) * es[u]->scale));
        for (int col = 0; col < G1; ++col) mx = std::max(mx, std::fabs(Wk(k, ev[u]->wbase + col) * ev[u]->scale));
      }
      eu[u] = pow2_above(mx);
    }
    auto Wg = [&](const UEntry* e, int u, int k, int col) { return e ? std::ldexp(Wk(k, e->wbase + col) * e->scale, -eu[u]) : 0.0; };
    std::vector<double> sc0(160, 1.0), sc1(32, 1.0);
    std::vector<float> cf0(160, 0.f), cf1(32, 0.f);
    for (int col = 0; col < G0; ++col) {
      double mx = 0;
      for (int k = 0; k < n_k; ++k) for (int u = 0; u < C; ++u) mx = std::max(mx, std::fabs(Wg(es[u], u, k, col)));
      const int sB = 14 - pow2_above(mx);
      sc0[col] = std::ldexp(1.0, sB); cf0[col] = (float)std::ldexp(1.0, -sB);
    }
    for (int col = 0; col < G1; ++col) {
      double mx = 0;
      for (int k = 0; k < n_k; ++k) for (int u = 0; u < C; ++u) mx = std::max(mx, std::fabs(Wg(ev[u], u, k, col)));
      const int sB = 14 - pow2_above(mx);
      sc1[col] = std::ldexp(1.0, sB); cf1[col] = (float)std::ldexp(1.0, -sB);
    }
    auto u_of = [](int t, int s2, int hh, int p) { return 32 * t + 16 * s2 + (p & 3) + 8 * (p >> 2) + 4 * hh; };
    std::vector<float4> wx((size_t)n_k * 48 * 64, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int k = 0; k < n_k; ++k)
      for (int lane = 0; lane < 64; ++lane) {
        const int hh = lane >> 5, c = lane & 31;
        for (int t = 0; t < 2; ++t)
          for (int s2 = 0; s2 < 2; ++s2) {
            for (int n = 0; n < 5; ++n) {
              const int col = 32 * n + c;
              double v[8];
              for (int pp = 0; pp < 8; ++pp) {
                const int u = u_of(t, s2, hh, pp);
                v[pp] = (u < C && col < G0) ? Wg(es[u], u, k, col) * sc0[col] : 0.0;
              }
              const size_t b = ((size_t)k * 48 + 20 * t + 2 * (2 * n + s2)) * 64 + lane;
              pack8(v, wx[b], wx[b + 64]);
            }
            double v[8];
            for (int pp = 0; pp < 8; ++pp) {
              const int u = u_of(t, s2, hh, pp);
              v[pp] = (u < C && c < G1) ? Wg(ev[u], u, k, c) * sc1[c] : 0.0;
            }
            const size_t b = ((size_t)k * 48 + 40 + 4 * t + 2 * s2) * 64 + lane;
            pack8(v, wx[b], wx[b + 64]);
          }
      }
    const size_t N = all_rows->size() / (size_t)row_len;
    double xm = 0;
    for (size_t i = 0; i < N; ++i)
      for (int u = 0; u < C; ++u) xm = std::max(xm, std::fabs(std::ldexp((double)(*all_rows)[i * row_len + u], eu[u])));
    L.x_sX = 14 - pow2_above(xm);
    const size_t n_pairs = (N + 1) / 2 + 96;  // a window reads up to 88 pairs (k_conv_mlx; k_conv_mfx: 32) from the pair of its first atom: zero rows behind the batch
    std::vector<unsigned> xph(n_pairs * 64, 0u), xpl(n_pairs * 64, 0u);
    for (size_t i = 0; i < N; ++i)
      for (int u = 0; u < C; ++u) {
        uint16_t hi, lo;
        split_f16(std::ldexp((double)(*all_rows)[i * row_len + u], eu[u] + L.x_sX), hi, lo);
        const size_t w = (i >> 1) * 64 + u;
        const int sh = (i & 1) ? 16 : 0;
        xph[w] |= (unsigned)hi << sh;
        xpl[w] |= (unsigned)lo << sh;
      }
    L.wx = mem.upload(wx);
    L.xph = mem.upload(xph); L.xpl = mem.upload(xpl);
    L.xcf0 = mem.upload(cf0); L.xcf1 = mem.upload(cf1);
  }

  build_layer_common(mem, m, prefix, in_blocks, s_in, L, in0, in1);
  return L;
}

// ---- head (EquivariantMLP, _mlp.py:84-114) and output gain (e3conv.py:134-135)
void pack_head(const jamun_model& m, jamun_sampler* s) {
  const int mul0 = m.hp.mul0, mul1 = m.hp.mul1, G0 = mul0 + mul1;
  const auto& Wl = m.get("output_head.0.lin.weight", (int64_t)mul0 * G0 + (int64_t)mul1 * mul1);
  const auto& Wo = m.get("output_head.1.weight", mul1);
  const auto& gain = m.get("output_gain", 1);
  std::vector<float> wg((size_t)mul0 * mul1), wv((size_t)mul1 * mul1), wo(mul1);
  for (int u = 0; u < mul0; ++u)
    for (int w = 0; w < mul1; ++w) wg[(size_t)u * mul1 + w] = (float)((double)Wl[(size_t)u * G0 + mul0 + w] / std::sqrt((double)mul0));
  for (int i = 0; i < mul1 * mul1; ++i) wv[i] = (float)((double)Wl[(size_t)mul0 * G0 + i] / std::sqrt((double)mul1));
  for (int w = 0; w < mul1; ++w) wo[w] = (float)((double)Wo[w] / std::sqrt((double)mul1) * (double)gain[0]);
  s->w_gate = s->mem.upload(wg); s->w_vec = s->mem.upload(wv); s->w_out = s->mem.upload(wo);
}

// f16x3 radial MLP (k_edge_h16): W1's radial part per layer scaled to the top of the f16 range and split hi + lo, as A fragments
void pack_edge_h16(jamun_sampler* s) {
  std::vector<float4> w1h;
  std::vector<float> isc;
  for (auto& L : s->layers) {
    double wmax = 0;
    for (float v : L.w1r_h) wmax = std::max(wmax, (double)std::fabs(v));
    int ex = 0;
    if (wmax > 0 && std::isfinite(wmax)) std::frexp(wmax, &ex);
    const int sW = std::max(-40, std::min(40, 14 - ex));
    isc.push_back((float)std::ldexp(1.0, -14 - sW));
    const double sc = std::ldexp(1.0, sW);
    for (int mt = 0; mt < 2; ++mt)
      for (int s2 = 0; s2 < 2; ++s2) {
        std::vector<float4> hi(64), lo(64);
        for (int lane = 0; lane < 64; ++lane) {
          const int hh = lane >> 5, k = 32 * mt + (lane & 31);
          double v[8];
          for (int j = 0; j < 8; ++j) v[j] = (double)L.w1r_h[(size_t)(16 * s2 + 8 * hh + j) * 64 + k] * sc;  // w1r: [basis][hidden]
          pack8(v, hi[lane], lo[lane]);
        }
        w1h.insert(w1h.end(), hi.begin(), hi.end());
        w1h.insert(w1h.end(), lo.begin(), lo.end());
      }
  }
  s->w1h_all = s->mem.upload(w1h); s->w1isc_all = s->mem.upload(isc);
}
