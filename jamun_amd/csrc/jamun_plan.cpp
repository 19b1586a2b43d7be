// jamun_plan.cpp — host planning behind jamun_sampler_create: the tiles and work lists of the destination-grouped conv kernels, and the
// selection of the kernels a sampler runs.  Pure host code: no HIP runtime call.
#include <cmath>

#include "jamun_host.h"

// Tiles of the destination-grouped conv kernels.  A tile = up to 32 consecutive destination atoms whose source span (whole
// molecules) has at most `cap` rows; tiles are cut greedily at molecule granularity.  A molecule larger than `cap`: its sources
// are cut into row blocks of <= cap atoms and every destination chunk (<= 32 atoms of the molecule) gets one tile PER source
// block — the contraction is linear in the edge coefficients, so the blocks' results are just more partial slabs for the node
// update to sum (edges whose source lies outside a tile's block are skipped by that tile).
void plan_tiles(const int32_t* ptr, const std::vector<int>& graph_of, int N, int cap, std::vector<int2>& t_atoms,
                std::vector<int2>& t_span, std::vector<int>& t_chunk, int& n_chunks, int& span_max, bool& row_blocks) {
  int a0 = 0;
  while (a0 < N) {
    const int g0 = graph_of[a0], lo = ptr[g0], mol_hi = ptr[g0 + 1];
    if (mol_hi - lo > cap) {
      const int n_mol = mol_hi - lo, nb = (n_mol + cap - 1) / cap;
      row_blocks = true;
      for (int d0 = lo; d0 < mol_hi; d0 += 32) {
        const int cnt = std::min(32, mol_hi - d0);
        for (int b = 0; b < nb; ++b) {
          const int blo = lo + (int)((int64_t)n_mol * b / nb), bhi = lo + (int)((int64_t)n_mol * (b + 1) / nb);
          t_atoms.push_back(make_int2(d0, cnt));
          t_span.push_back(make_int2(blo, bhi));
          t_chunk.push_back(n_chunks);
          span_max = std::max(span_max, bhi - blo);
        }
        ++n_chunks;
      }
      a0 = mol_hi;
      continue;
    }
    int cnt = 0, hi = lo;
    while (a0 + cnt < N && cnt < 32) {
      const int g2 = graph_of[a0 + cnt], nhi = ptr[g2 + 1];
      if (nhi - lo > cap) break;  // (also stops in front of a molecule that needs row blocks)
      cnt += std::min(nhi - (a0 + cnt), 32 - cnt);
      hi = nhi;
    }
    t_atoms.push_back(make_int2(a0, cnt));
    t_span.push_back(make_int2(lo, hi));
    t_chunk.push_back(n_chunks++);
    span_max = std::max(span_max, hi - lo);
    a0 += cnt;
  }
}

// Work lists of the persistent conv kernels.  Work items are (tile, hidden unit k).  k is sliced over `ng` groups of XCDs
// (workgroup g runs on XCD g % 8, so an XCD's L2 holds only its slice of the weights); the n_k % ng left-over k are dealt
// round-robin over (tile, slice).  Each slice's item list (tile-major) is cut over its workgroups — evenly by item count for
// near-uniform batches, by modelled cost otherwise: a workgroup gets a few runs of k ("segments"), each written to its own
// partial slab of the tile's destination chunk.
SegPlan plan_segments(int cus, int ng, int n_k, int N, const std::vector<int2>& t_atoms, const std::vector<int>& t_chunk, int n_chunks,
                      const std::vector<int64_t>& tile_weight, const std::vector<char>* skip,  // skip[t]: tile t is not on this plan (its atoms get 0 slabs)
                      double seg_cost) {                                                       // cost of a segment's prologue + epilogue, in items
  SegPlan P;
  auto weight = [&](int t) { return tile_weight[t]; };
  const int ncx_all = cus / ng;
  std::vector<std::vector<int>> wg_of(ng);  // workgroups of k-slice x, in launch order
  for (int g = 0; g < cus; ++g) wg_of[ng == 1 ? 0 : (g % 8) % ng].push_back(g);
  const int base = n_k / ng, rem = n_k % ng;
  std::vector<std::vector<int4>> wg_segs(cus);
  const int n_tiles = (int)t_atoms.size();
  std::vector<int> nslab(n_chunks, 0);  // per destination chunk: its tiles (source row blocks, k runs) number their slabs jointly
  for (int x = 0; x < ng; ++x) {
    auto extra_of = [&](int t) { const int e = ((x - t) % ng + ng) % ng; return e < rem ? ng * base + e : -1; };
    // (near-uniform batches are cut by item count: measured 1 % better on cfg2 than the modelled weights, whose error
    // then exceeds the spread they describe)
    auto skipped = [&](int t) { return skip && (*skip)[t]; };
    int64_t w_min = -1, w_max = -1;
    for (int t = 0; t < n_tiles; ++t) {
      if (skipped(t)) continue;
      w_min = w_min < 0 ? weight(t) : std::min<int64_t>(w_min, weight(t));
      w_max = std::max<int64_t>(w_max, weight(t));
    }
    if (w_max < 0) continue;  // (no tile on this plan)
    const bool uniform = 4 * (w_max - w_min) < w_max;
    auto weight_of = [&](int t) -> int64_t { return uniform ? 1 : weight(t); };
    const double unit = uniform ? 1.0 : 1.0 / (double)std::max<int64_t>(w_min, 1);
    int64_t Lx = 0, Wx = 0;
    for (int t = 0; t < n_tiles; ++t) {
      if (skipped(t)) continue;
      const int cnt = base + (extra_of(t) >= 0 ? 1 : 0);
      Lx += cnt;
      Wx += cnt * weight_of(t);
    }
    // small batches: do not cut the list finer than 8 items per workgroup (a tile's partial slabs are summed by the node
    // update; one slab per hidden unit would make that kernel the bottleneck)
    const int ncx = (int)std::max<int64_t>(1, std::min<int64_t>(ncx_all, Lx / 8));
    // Every segment costs its workgroup a prologue and an epilogue (staging the span's rows, the edge records, the partial slab): `seg_cost`
    // items' worth (measured with the kernels' segment stamps: k_conv_mf 17 k cycles against 4.75 k per item, k_conv_ml 49 k against 8.5 k).  A
    // workgroup whose share of the list crosses a tile boundary runs two segments, one that does not runs one: the list is cut so that
    // items x weight + segments x seg_cost is level — the smallest per-workgroup budget for which a greedy walk over the list fits ncx workgroups.
    auto walk = [&](double budget, std::vector<std::vector<int4>>* out) {
      int c = 0;
      double acc = 0;
      for (int t = 0; t < n_tiles; ++t) {
        if (skipped(t)) continue;
        const int ex = extra_of(t), cnt = base + (ex >= 0 ? 1 : 0);
        const double w = (double)weight_of(t) * unit;
        int i0 = 0;
        while (i0 < cnt) {
          // (the room in double: a wide budget over a light tile's weight exceeds the int range)
          const double room = std::floor((budget - acc - seg_cost) / w + 1e-9);
          if (room < 1 && acc > 0) { ++c; acc = 0; continue; }  // (no room for a segment with one item: next workgroup)
          const int take = room < 1 ? 1 : (int)std::min<double>(room, cnt - i0);
          if (c >= ncx) return false;
          if (out) {
            const int i1 = i0 + take;
            const int kb = x * base + std::min(i0, base), ke = x * base + std::min(i1, base);
            auto& v = (*out)[c];
            v.push_back(make_int4(t, nslab[t_chunk[t]]++, kb, ke));
            v.push_back(make_int4(i1 > base ? ex : -1, 0, 0, 0));
          }
          acc += seg_cost + take * w;
          i0 += take;
        }
      }
      return c < ncx;
    };
    double lo = 0, hi = 0;
    {
      // unit: items are counted in units of the lightest tile's weight
      for (int t = 0; t < n_tiles; ++t)
        if (!skipped(t)) hi += (base + (extra_of(t) >= 0 ? 1 : 0)) * (double)weight_of(t) * unit + seg_cost;
      lo = hi / ncx * 0.5;
    }
    for (int iter = 0; iter < 60; ++iter) {
      const double mid = 0.5 * (lo + hi);
      if (walk(mid, nullptr)) hi = mid; else lo = mid;
    }
    // Which workgroup runs which share.  Workgroup g runs on XCD g % 8 (round-robin dispatch), every XCD has its own 4 MB L2, and every
    // workgroup streams the layer's weights (127 KB per hidden unit) at the pace of its k loop: a block is served by the L2 a second
    // time only to a workgroup of the SAME XCD that reaches the same hidden unit within a few steps (32 streams x 127 KB = the whole L2
    // per step).  The shares are therefore dealt to the XCDs by the PHASE of their k loop — the hidden unit their first segment starts
    // at; a share continues with k = 0 of the next tile when it crosses a tile boundary —: the 32 workgroups of an XCD then walk a
    // window of ~65 / 8 hidden units together, ~1 MB of weights, and every XCD fetches the stream once (cfg2: FETCH_SIZE of k_conv_mf
    // 291 -> 90 MB per launch, +2.3 % conformations/s; cfg5 +1.5 %; in launch order the phases of an XCD's workgroups were spread over
    // all 65 units — profiles/EXPERIMENTS.md).
    // (the greedy walk is not strictly monotone in the budget: the bisection's `hi` is verified, and widened if need be, BEFORE the walk that
    // numbers the slabs — the first budget tried above, the whole list in one share, always fits)
    for (int grow = 0; grow < 64 && !walk(hi, nullptr); ++grow) hi *= 1.05;
    std::vector<std::vector<int4>> share((size_t)ncx);
    if (!walk(hi, &share)) throw Err(JAMUN_ERR_INVALID, "plan_segments: no feasible cut of the work list");
    {  // every (tile, hidden unit) of this plan exactly once
      std::vector<int> covered((size_t)n_tiles, 0), extra_seen((size_t)n_tiles, 0);
      for (auto& v : share)
        for (size_t q = 0; q + 1 < v.size(); q += 2) {
          covered[v[q].x] += v[q].w - v[q].z;
          if (v[q + 1].x >= 0) ++extra_seen[v[q].x];
        }
      for (int t = 0; t < n_tiles; ++t) {
        if (skipped(t)) continue;
        if (covered[t] != base || extra_seen[t] != (extra_of(t) >= 0 ? 1 : 0)) throw Err(JAMUN_ERR_INVALID, "plan_segments: a tile's hidden units are not covered exactly once");
      }
    }
    std::vector<int> order;
    for (int c = 0; c < ncx; ++c)
      if (!share[c].empty()) order.push_back(c);
    const int kspan = std::max(1, base + (rem ? 1 : 0));
    auto phase = [&](int c) { return ((share[c][0].z - x * base) % kspan + kspan) % kspan; };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return phase(a) < phase(b); });
    std::vector<std::vector<int>> by_xcd(8);
    for (int g : wg_of[x]) by_xcd[g % 8].push_back(g);
    std::vector<int> xcds;
    for (int q = 0; q < 8; ++q)
      if (!by_xcd[q].empty()) xcds.push_back(q);
    // (equal counts per XCD, the remainder to the first ones — the shares are level, so are the XCDs)
    size_t pos = 0;
    for (size_t qi = 0; qi < xcds.size(); ++qi) {
      const size_t n_q = order.size() / xcds.size() + (qi < order.size() % xcds.size() ? 1 : 0);
      auto& ids = by_xcd[xcds[qi]];
      for (size_t j = 0; j < n_q && pos < order.size(); ++j, ++pos) {
        if (j >= ids.size()) throw Err(JAMUN_ERR_INVALID, "plan_segments: more shares than workgroups on an XCD");
        wg_segs[ids[j]] = share[order[pos]];
      }
    }
  }
  size_t ms = 1;
  for (auto& v : wg_segs) ms = std::max(ms, v.size() / 2 + 1);
  P.max_segs = (int)ms;
  P.segs.assign((size_t)cus * ms * 2, make_int4(-1, 0, 0, 0));
  for (int g = 0; g < cus; ++g) std::copy(wg_segs[g].begin(), wg_segs[g].end(), P.segs.begin() + (size_t)g * ms * 2);
  for (int v : nslab) P.n_slabs = std::max(P.n_slabs, v);
  P.atom_nslab.assign(N, 1);
  for (int t = 0; t < n_tiles; ++t)
    for (int i = 0; i < t_atoms[t].y; ++i) P.atom_nslab[t_atoms[t].x + i] = nslab[t_chunk[t]];
  return P;
}

// validates ptr and the bond list, builds the bonded-edge CSR, derives the edge stride S
TopoHost check_topology(const jamun_topology& topo) {
  const int N = topo.n_atoms, W = topo.n_graphs;
  TopoHost t;
  for (int g = 0; g < W; ++g) {
    if (topo.ptr[g + 1] < topo.ptr[g]) throw Err(JAMUN_ERR_INVALID, "ptr must be non-decreasing");
    t.nmax = std::max(t.nmax, topo.ptr[g + 1] - topo.ptr[g]);
  }
  if (topo.ptr[0] != 0 || topo.ptr[W] != N) throw Err(JAMUN_ERR_INVALID, "ptr must span [0, n_atoms]");
  t.graph_of.resize(N);
  for (int g = 0; g < W; ++g)
    for (int a = topo.ptr[g]; a < topo.ptr[g + 1]; ++a) t.graph_of[a] = g;
  t.bip.assign(N + 1, 0);
  t.bis.resize(topo.n_bonds);
  for (int b = 0; b < topo.n_bonds; ++b) {
    const int64_t sa = topo.bond_src[b], da = topo.bond_dst[b];
    if (sa < 0 || sa >= N || da < 0 || da >= N) throw Err(JAMUN_ERR_INVALID, "bond index out of range");
    if (t.graph_of[sa] != t.graph_of[da]) throw Err(JAMUN_ERR_INVALID, "bond connects two different walkers");
    t.bip[da + 1]++;
  }
  int max_in = 0;
  for (int i = 0; i < N; ++i) { max_in = std::max(max_in, t.bip[i + 1]); t.bip[i + 1] += t.bip[i]; }
  std::vector<int> fill(t.bip.begin(), t.bip.end() - 1);
  for (int b = 0; b < topo.n_bonds; ++b) t.bis[fill[topo.bond_dst[b]]++] = (int)topo.bond_src[b];  // stable: list order
  t.S = std::max(1, std::min(std::max(t.nmax - 1, 0), JAMUN_MAX_NEIGHBORS + 1) + max_in);
  return t;
}

// Which of the two families a model's layers run on before any tile plan is looked at: Conv models outside the envelope of the compiled-width
// kernels take the wide path (jamun_wide.hip); every model inside it selects exactly the kernels it selected before the wide path existed
ConvPath base_conv_path(const jamun_hparams& hp, int n_emb) {
  const bool outside = hp.edge_attr_dim != 64 || (hp.mul0 + hp.mul1 + 31) / 32 > 5 || (hp.mul1 + 31) / 32 > 2 || n_emb > 224 ||
                       hp.mul0 + 3 * hp.mul1 > 224 || hp.mul0 + hp.mul1 > 160 || hp.mul1 > 32;
  if (outside && hp.separable)
    throw Err(JAMUN_ERR_INVALID, "irreps too wide for the node-update tiling (embedding <= 224, hidden <= 160 channels, <= 32 vectors)");
  return outside ? CONV_WIDE : hp.separable ? CONV_SEP : CONV_GENERAL;
}

// ---- kernel selection of jamun_sampler_create, in stages: each a function of the inputs and of the plan so far ---------------------
namespace {

struct SelectIn {
  const jamun_hparams& hp;
  const jamun_tuning& tn;
  const jamun_topology& topo;
  const TopoHost& th;
  int cus;
  const PackedLayouts& lay;
  int n_uniq;
  bool have_atom_uid;
  int N() const { return topo.n_atoms; }
  int n_k() const { return hp.edge_attr_dim + 1; }
  int pmax() const { return (th.S + 3) & ~3; }
  bool mf_packed() const { return !lay.hidden.empty() && lay.hidden[0].mf; }
  bool tail_packed() const { return !lay.hidden.empty() && lay.hidden[0].tail; }
};

// Stage 1, the tile plan and the hidden layers' kernel: the destination-grouped kernels (own tile plan, larger spans) when the model, the
// batch and the packed weights allow them, and of those the fastest whose span budget does not cost too many tiles.  false: no tile plan.
bool select_tiles(const SelectIn& in, KernelPlan& sel) {
  const jamun_tuning& tn = in.tn;
  const int N = in.N(), S = in.th.S;
  bool ok = !tn.no_dg && sel.conv_path == CONV_GENERAL && in.hp.n_layers > 0 && S <= 64 && (int64_t)N * S < (int64_t)0x7fffffff;
  for (const PackedLayouts::Hidden& h : in.lay.hidden) ok = ok && h.dg;
  // Source rows resident in LDS for the whole segment when the largest molecule fits the resident budget (~80 rows);
  // otherwise the alternating-residency mode of the kernel (rows re-staged per phase: spans up to ~170 rows), and only
  // molecules above THAT are cut into source row blocks.
  auto cap_of = [&](DgMode mode) {
    for (int rs = mode == DG_ALT ? 192 : 128; rs >= 16; rs -= 4)
      if (conv_dg_lds_bytes(rs, in.pmax(), mode, sel.dg_emu) <= JAMUN_MAX_DYN_LDS) return rs;
    return 0;
  };
  int cap = ok ? cap_of(DG_RESIDENT) : 0;
  DgMode mode = DG_RESIDENT;
  if (ok && in.th.nmax > cap && !tn.dg_no_alt) {
    const int cap_alt = cap_of(DG_ALT);
    if (cap_alt > cap) { cap = cap_alt; mode = DG_ALT; }
  }
  if (!ok || cap <= 0) return false;
  sel.conv_path = CONV_DG;
  TilePlan& T = sel.tiles;
  // One trial: plan the tiles at span budget `c` and take the plan, as kernel mode `m`, if `accept` says so
  auto try_plan = [&](int c, DgMode m, auto accept) {
    TilePlan q;
    plan_tiles(in.topo.ptr, in.th.graph_of, N, c, q.atoms, q.span, q.chunk, q.n_chunks, q.span_max, q.row_blocks);
    if (!accept(q)) return;
    T = std::move(q);
    sel.dg_mode = m;
  };
  // (a smaller budget: no source row blocks, and at most pct % of the tiles of the plan at hand)
  auto costs_at_most = [&](size_t pct) { return [&T, pct](const TilePlan& q) { return !q.row_blocks && 100 * q.atoms.size() <= pct * T.atoms.size(); }; };
  try_plan(cap, mode, [](const TilePlan&) { return true; });
  // single phase with double-buffered A tiles (spans up to ~52 rows) when the smaller span budget does not cost tiles (17-atom molecules:
  // three per tile either way; a 40-atom molecule would fall from straddling tiles to 32 + 8 destinations)
  if (sel.dg_mode == DG_RESIDENT && cap_of(DG_SINGLE) >= 16 && !tn.dg_no_sp) try_plan(cap_of(DG_SINGLE), DG_SINGLE, costs_at_most(103));
  // single phase with a double-buffered X tile and ONE Y tile (spans up to ~73 rows: two 33-atom molecules per tile) when the
  // fully double-buffered variant does not fit: a k-step of the two-phase kernel takes 25 k cycles on such tiles, of this
  // one ~17 k, so up to 15 % more tiles are accepted
  if (sel.dg_mode == DG_RESIDENT && cap_of(DG_SINGLE_Y) >= 16 && !tn.dg_no_sph) try_plan(cap_of(DG_SINGLE_Y), DG_SINGLE_Y, costs_at_most(115));
  const bool mf_ok = sel.dg_emu && !tn.no_mf && in.mf_packed();  // (the matrix-formed kernels: f16x3 only)
  // (the edges of one ordered pair share one coefficient entry, owned by the first with up to two more added: radial edge +
  // at most two listings of the bond)
  int mult = 0;
  if (mf_ok) {
    std::vector<std::pair<int64_t, int64_t>> bb;
    for (int b = 0; b < in.topo.n_bonds; ++b) bb.push_back({in.topo.bond_src[b], in.topo.bond_dst[b]});
    std::sort(bb.begin(), bb.end());
    for (size_t i = 0, j = 0; i < bb.size(); i = j) {
      while (j < bb.size() && bb[j] == bb[i]) ++j;
      mult = std::max(mult, (int)(j - i));
    }
  }
  // A operand formed on the matrix cores (jamun_conv_mf.hip): spans that fit one K = 64 window of source rows (from an even
  // atom: 62 rows), when that budget costs no tiles
  // (measured per (tile, k) and workgroup: 3.7 us here, 5.7 us single-phase k_conv_dg, 9.5 us its one-Y-tile variant: the smaller
  // span budget may cost tiles — 33-atom molecules go from two per tile pair to 32 + 1 destinations)
  if (mf_may_replace(sel.dg_mode) && mf_ok)
    try_plan(62, DG_MF, [&, within = costs_at_most(sel.dg_mode == DG_SINGLE ? 140 : 230)](const TilePlan& q) { return within(q) && q.span_max <= 62 && mult <= 2; });
  // ... and for larger spans (molecules of 63 .. 167 atoms) the two-pass, block-sparse variant jamun_conv_ml.hip: whole molecules as
  // spans of up to 167 rows; edge strides 33..40 (32 radial slots + bonded in-edges)
  if (ml_may_replace(sel.dg_mode) && mf_ok && !tn.no_ml && S >= 33 && S <= 40)
    try_plan(167, DG_ML, [&](const TilePlan& q) {
      int need = 0;
      for (auto& sp : q.span) need = std::max(need, sp.y - (sp.x & ~1));
      const int window = conv_ml_window(need);
      if (q.row_blocks || window <= 0 || mult > 2 || (int64_t)in.n_k() * 32 * (((int64_t)N + 31 & ~31) + 64) * 4 >= ((int64_t)1 << 40)) return false;
      sel.ml_window = window;
      return true;
    });
  sel.dg_RS = std::max((T.span_max + 3) & ~3, 16);  // (>= 16 rows: the segment-end staging tile of the forming waves aliases the source rows)
  return true;
}

// Stage 2, tail tiles (DG_MF): a tile with at most 8 destinations costs k_conv_mf a whole tile per hidden unit (a 33-atom molecule cuts into
// 32 + 1: twice the work of a 32-atom one).  They leave the hidden layers' segment lists and go through k_tail_form /
// k_tail_contract (jamun_conv_tail.hip); worth two more launches per layer when they are at least 4 and 3 % of the tiles.
// Returns which tiles are tail tiles; also fixes the forming K-steps of the whole tiles.
std::vector<char> select_tail_tiles(const SelectIn& in, KernelPlan& sel) {
  const TilePlan& T = sel.tiles;
  std::vector<char> is_tail(T.atoms.size(), 0);
  if (sel.dg_mode == DG_MF && !in.tn.no_tail && in.tail_packed()) {
    std::vector<int4> tt;
    std::vector<int> tatom;
    for (size_t t = 0; t < T.atoms.size(); ++t)
      if (T.atoms[t].y <= 8) {
        tt.push_back(make_int4((int)t, (int)tatom.size(), 0, 0));
        for (int i = 0; i < T.atoms[t].y; ++i) tatom.push_back(T.atoms[t].x + i);
      }
    const size_t p_bytes = (size_t)((tatom.size() + 31) / 32) * 32 * (size_t)in.n_k() * TAIL_NFT * 8 * 16;
    if (tt.size() >= 4 && 100 * tt.size() >= 3 * T.atoms.size() && tt.size() < T.atoms.size() && p_bytes <= ((size_t)2 << 30)) {
      for (auto& e : tt) {
        is_tail[e.x] = 1;
        // (the record carries its tile's descriptor — {first tail destination, first atom, atoms | source rows << 8, first source row} —
        // so that the tail kernels do not start with a second, dependent trip to the tile tables; as the segment records of k_conv_mf)
        const int t = e.x;
        e = make_int4(e.y, T.atoms[t].x, T.atoms[t].y | ((T.span[t].y - T.span[t].x) << 8), T.span[t].x);
      }
      const int n_ct = ((int)tatom.size() + 31) / 32;
      // runs of hidden units of the contraction = partial slabs of the tail atoms: one workgroup per (32 destinations, run, output
      // tile); the node update fetches three slabs at once, so at most three
      sel.tail_runs = std::max(1, std::min(3, (32 + n_ct - 1) / n_ct));
      sel.tail_tiles = std::move(tt);
      sel.tail_atom = std::move(tatom);
      sel.tail_P_bytes = p_bytes;
    }
  }
  if (matrix_formed(sel.dg_mode)) {
    int need = 0;  // rows of the window a tile's sources reach (the window starts at an even atom)
    for (size_t t = 0; t < T.span.size(); ++t)
      if (!is_tail[t]) need = std::max(need, T.span[t].y - (T.span[t].x & ~1));
    sel.mf_nks = (need <= 48 && !in.tn.no_short_k) ? 3 : 4;
  }
  return is_tail;
}

// Stage 3, the work lists: the hidden layers' without the tail tiles, and the initial projector's own when it keeps those as tiles
void plan_work_lists(const SelectIn& in, KernelPlan& sel, const std::vector<char>& is_tail) {
  const jamun_tuning& tn = in.tn;
  const TilePlan& T = sel.tiles;
  const int N = in.N(), n_k = in.n_k();
  // k-slices over XCD groups (jamun_tuning.dg_kgroups = 1, 2, 4, 8).  Measured on MI355X (cfg2, profiles/r2*): 1 slice 0.317 ms per
  // launch, 2: 0.318, 4: 0.328, 8: 0.343 and the node update slows from 25 to 71 us (more partial slabs per tile): the
  // ~7.7 MB of weight blocks per layer are served from L2 / Infinity Cache fast enough, longer runs of k per segment win.
  sel.ng = (tn.dg_kgroups > 1 && in.cus % 8 == 0 && n_k >= tn.dg_kgroups) ? tn.dg_kgroups : 1;
  std::vector<int64_t> weight(T.atoms.size());
  for (size_t t = 0; t < weight.size(); ++t) weight[t] = 476 + (sel.dg_mode == DG_ALT ? 24 : 2) * ((T.span[t].y - T.span[t].x + 15) / 16);
  const bool tails = !sel.tail_tiles.empty();
  // (a segment's prologue + epilogue in items of its k loop, from the kernels' segment stamps; jamun_tuning.seg_cost_tenths overrides)
  sel.seg_cost = tn.seg_cost_tenths < 0 ? 0.0 : tn.seg_cost_tenths > 0 ? 0.1 * tn.seg_cost_tenths : sel.dg_mode == DG_MF ? 3.6 : sel.dg_mode == DG_ML ? 5.8 : 0.0;
  sel.segs = plan_segments(in.cus, sel.ng, n_k, N, T.atoms, T.chunk, T.n_chunks, weight, tails ? &is_tail : nullptr, sel.seg_cost);
  if (!tails) return;
  for (size_t t = 0; t < T.atoms.size(); ++t)
    if (is_tail[t])
      for (int i = 0; i < T.atoms[t].y; ++i) sel.segs.atom_nslab[T.atoms[t].x + i] = sel.tail_runs;
  sel.segs.n_slabs = std::max(sel.segs.n_slabs, sel.tail_runs);
  sel.init_tail = in.lay.wx && in.lay.nt0 == 5 && !tn.no_mfi;
  if (!sel.init_tail) {  // the initial projector keeps every tile on segment lists of its own
    sel.init_segs = plan_segments(in.cus, sel.ng, n_k, N, T.atoms, T.chunk, T.n_chunks, weight, nullptr, sel.seg_cost);
    sel.own_init_segs = true;
  }
}

// Stage 4, the initial projector on the same tiles
void select_init_path(const SelectIn& in, KernelPlan& sel) {
  const jamun_tuning& tn = in.tn;
  const PackedLayouts& lay = in.lay;
  // k_conv_init_v: two LDS buffers of table rows when they fit (spans up to ~90 rows), else one (up to ~170 rows)
  // (mid-size ragged batches keep the MFMA table kernel: on 17-57 atom molecules, mean in-degree 11, it takes 0.283 ms
  // against 0.312 — the per-k staging of ~76 table rows outweighs the few edges; 33-atom molecules: 0.398 against 0.328)
  if (!tn.no_init_v && !sel.tiles.row_blocks && lay.tt2 && lay.nt0 == 5 && sel.dg_RS <= 170) {
    // (one buffer only for the large-molecule plan: measured on the ragged 17-57 atom batch the MFMA table kernel is 10 %
    // faster than the one-buffer variant, on 166-atom molecules — where it falls back to source row blocks — 2.1x slower)
    for (int nbuf = 2; nbuf >= ((sel.dg_mode == DG_ALT || sel.dg_mode == DG_ML) ? 1 : 2) && sel.init_path != INIT_V; --nbuf)
      if (conv_initv_lds_bytes(sel.dg_RS, in.pmax(), nbuf) <= JAMUN_MAX_DYN_LDS) { sel.init_path = INIT_V; sel.initv_nbuf = nbuf; }
  }
  // ... or, on the tiles of k_conv_mf (spans within one K = 64 window) and with at most 32 distinct embedding rows, the same
  // scheme with a one-hot selector in place of the feature rows (k_conv_mfi)
  if (sel.dg_mode == DG_MF && lay.nt0 == 5 && !tn.no_mfi) {
    // up to 32 distinct rows: one selector tile (112 MFMAs per (tile, k), eight equal waves); more: from the feature rows (192)
    if (in.n_uniq <= 32 && lay.tabw && in.have_atom_uid && lay.tab_ut == 1) sel.init_path = INIT_MFI;
    else if (lay.wx) sel.init_path = INIT_MFX;
  }
  if (sel.dg_mode == DG_ML && lay.nt0 == 5 && !tn.no_mfi && lay.wx) sel.init_path = INIT_MLX;
}

}  // namespace

// The conv kernel of the hidden layers, the kernel of the initial projector, and the tile plan and work lists they run on.  Depends on the
// model, the tuning switches, the batch's molecule sizes and bonds, the edge stride, the number of CUs and on which weight layouts packing
// produced; touches no device memory.
KernelPlan select_kernels(const jamun_hparams& hp, const jamun_tuning& tn, const jamun_topology& topo, const TopoHost& th, int cus, ConvPath base,
                          const PackedLayouts& lay, int n_uniq, bool have_atom_uid) {
  const SelectIn in{hp, tn, topo, th, cus, lay, n_uniq, have_atom_uid};
  KernelPlan sel;
  sel.conv_path = base;
  sel.init_path = base == CONV_WIDE ? INIT_WIDE : base == CONV_SEP ? INIT_SEP : INIT_GENERAL;
  sel.dg_emu = tn.dg_fp32 ? 0 : 1;
  if (!select_tiles(in, sel)) return sel;
  const std::vector<char> is_tail = select_tail_tiles(in, sel);
  plan_work_lists(in, sel, is_tail);
  select_init_path(in, sel);
  return sel;
}

// per (tile, k) in k_conv_dg: fp32 path 476 units of v_mfma_f32_32x32x2 (4096 FLOP); f16x3 path 150 v_mfma_f32_32x32x16_f16
// (32768 FLOP: 50 groups of 16 inputs x 3 products) + 72 v_mfma_f32_16x16x32_f16 (16384 FLOP); + 60 fp32 units per (32 atoms, k)
// in the T pre-pass
// (k_conv_mf: 414 v_mfma_f32_32x32x16_f16 per (tile, k): 228 forming + 186 contraction; k_conv_ml: 57 forming per 16 rows of its window)
ConvModel conv_model(const KernelPlan& plan, const jamun_hparams& hp, int n_atoms) {
  ConvModel m;
  if (plan.conv_path != CONV_DG) return m;
  const int64_t n_k = hp.edge_attr_dim + 1;
  int64_t per_tile_k = 476LL * 4096, w_blocks = 5 * 16 + 5 * 4 + 2 * 4;  // (weights: 64-lane float4 blocks per hidden unit)
  if (plan.dg_emu) { per_tile_k = 150LL * 32768 + 72LL * 16384; w_blocks = 4 * 34; }
  if (plan.dg_mode == DG_MF) per_tile_k = (plan.mf_nks == 3 ? 357LL : 414LL) * 32768;
  if (plan.dg_mode == DG_ML) per_tile_k = (57LL * ((plan.ml_window + 15) / 16) + 186) * 32768;
  if (matrix_formed(plan.dg_mode)) w_blocks = 124;
  m.conv_flop = (int64_t)(plan.tiles.atoms.size() - plan.tail_tiles.size()) * per_tile_k * n_k;  // (tail tiles run in their own kernels)
  m.tprod_flop = (int64_t)((n_atoms + 31) / 32) * (plan.dg_emu ? 24LL * 32768 : 60LL * 4096) * n_k;
  m.weight_bytes = n_k * w_blocks * 64 * 16;
  return m;
}
