"""CPU tests: the work-list planner of the destination-grouped conv kernels (``plan_segments`` in jamun_plan.cpp, reached through
``jamun_debug_plan_segments``) keeps its invariants under every plan the host can emit — k-slices over XCD groups (jamun_tuning.dg_kgroups),
the segment cost (jamun_tuning.seg_cost_tenths), non-uniform tile weights, source row blocks sharing a destination chunk, skipped (tail) tiles.

``check_plan`` is also what tests/test_gpu_plans.py runs on the lists a live sampler's kernels read."""
import math
import random

import numpy as np
import pytest

FORMS = ("k_extra", "k_run0", "multi_seg", "slabs_gt3")


def check_plan(segs, *, cus, ng, n_k, n_atoms, tiles, chunk, max_segs, n_slabs, atom_nslab, skip=None, weights=None, seg_cost=None,
               skipped_nslab=None, spans=None):
    """Assert the invariants of one plan; return the set of rare forms (FORMS) it contains.

    segs [cus, max_segs, 2, 4] int32: {tile, slab, k_begin, k_end}, {k_extra, ...}.  tiles [n_tiles, 2] {first atom, atoms}; chunk [n_tiles]
    destination chunk; skip [n_tiles] tiles not on this plan.  weights + seg_cost: also check the balance of the cut.  skipped_nslab: the
    slab count the sampler gives atoms of skipped tiles (tail runs; None: the planner's own 0).  spans [n_tiles, 2]: the tile descriptor the
    sampler embeds into the second record is checked against it."""
    segs = np.asarray(segs, dtype=np.int64)
    tiles = np.asarray(tiles, dtype=np.int64).reshape(-1, 2)
    chunk = np.asarray(chunk, dtype=np.int64)
    n_tiles = tiles.shape[0]
    skip = np.zeros(n_tiles, bool) if skip is None else np.asarray(skip).astype(bool)
    assert segs.shape == (cus, max_segs, 2, 4), (segs.shape, cus, max_segs)
    base, rem = n_k // ng, n_k % ng
    r0, r1 = segs[:, :, 0, :], segs[:, :, 1, :]
    valid = r0[..., 0] >= 0
    # padding: every workgroup's list is a prefix of records, the rest exactly {-1, 0, 0, 0} twice
    assert np.all(valid[:, 1:] <= valid[:, :-1]), "a real record after a padding record"
    pad = ~valid
    assert np.all(r0[pad] == np.array([-1, 0, 0, 0])) and np.all(r1[pad] == np.array([-1, 0, 0, 0])), "padding records are not {-1, 0, 0, 0}"
    nseg = valid.sum(1)
    assert nseg.max(initial=0) <= max_segs
    assert max_segs == max(1, int(nseg.max(initial=0)) + 1), (max_segs, nseg.max(initial=0))  # (as the planner sizes the lists: one terminator)
    g = np.repeat(np.arange(cus), max_segs).reshape(cus, max_segs)[valid]
    t, slab, kb, ke, ex = r0[valid][:, 0], r0[valid][:, 1], r0[valid][:, 2], r0[valid][:, 3], r1[valid][:, 0]
    assert np.all(t < n_tiles), "tile index out of range"
    assert not np.any(skip[t]), "a skipped tile on the plan"
    # XCD weight slices: workgroup g runs on XCD g % 8 and holds segments of slice (g % 8) % ng only
    x = (g % 8) % ng if ng > 1 else np.zeros_like(g)
    assert np.all((kb >= x * base) & (kb <= ke) & (ke <= (x + 1) * base)), "a k run outside its workgroup's slice"
    has_ex = ex >= 0
    e = (x - t) % ng
    assert np.all(ex[has_ex] == ng * base + e[has_ex]) and np.all(e[has_ex] < rem), "k_extra is not the slice's left-over unit of the tile"
    assert np.all(ex[~has_ex] == -1)
    assert np.all((ke > kb) | has_ex), "a segment without work"
    # every hidden unit of every tile on the plan exactly once
    cov = np.zeros((n_tiles, n_k + 1), np.int64)
    np.add.at(cov, (t, kb), 1)
    np.add.at(cov, (t, ke), -1)
    cov = np.cumsum(cov, axis=1)[:, :n_k]
    np.add.at(cov, (t[has_ex], ex[has_ex]), 1)
    want = np.where(skip[:, None], 0, 1)
    bad = np.argwhere(cov != want)
    assert bad.size == 0, f"(tile, hidden unit) covered {cov[tuple(bad[0])]} times: {bad[:4].tolist()}"
    # partial slabs: within a destination chunk ids 0..count-1, each once
    n_chunks = int(chunk.max()) + 1 if n_tiles else 0
    c = chunk[t]
    count = np.bincount(c, minlength=n_chunks)
    key = c * (int(slab.max(initial=0)) + 1) + slab
    assert np.all(slab >= 0) and np.unique(key).size == key.size, "a slab id used twice within a destination chunk"
    top = np.full(n_chunks, -1)
    np.maximum.at(top, c, slab)
    assert np.all(top + 1 == count), "slab ids of a chunk are not 0..count-1"
    exp_nslab = max(1, int(count.max(initial=0)))
    if skipped_nslab is not None and skip.any():
        exp_nslab = max(exp_nslab, skipped_nslab)
    assert n_slabs == exp_nslab, (n_slabs, exp_nslab)
    exp_atom = np.ones(n_atoms, np.int64)
    val = count[chunk] if skipped_nslab is None else np.where(skip, skipped_nslab, count[chunk])
    n_of = tiles[:, 1]
    idx = np.repeat(tiles[:, 0], n_of) + np.arange(int(n_of.sum())) - np.repeat(np.cumsum(n_of) - n_of, n_of)
    exp_atom[idx] = np.repeat(val, n_of)  # (tiles in order, the last one of an atom wins: as the planner writes them)
    assert np.array_equal(np.asarray(atom_nslab, np.int64), exp_atom), "atom_nslab differs from the chunk's slab count"
    if spans is not None:  # (the sampler's copy of the tile descriptor in the second record: {k_extra, first atom, atoms | rows << 8, first row})
        spans = np.asarray(spans, np.int64).reshape(-1, 2)
        assert np.array_equal(r1[valid][:, 1], tiles[t, 0]) and np.array_equal(r1[valid][:, 3], spans[t, 0])
        assert np.array_equal(r1[valid][:, 2], tiles[t, 1] | ((spans[t, 1] - spans[t, 0]) << 8))
    if weights is not None:
        _check_balance(cus, ng, base, rem, n_tiles, skip, np.asarray(weights, np.float64), float(seg_cost), g, x, t, kb, ke, has_ex)
    forms = set()
    if has_ex.any():
        forms.add("k_extra")
    if np.any((kb == ke) & has_ex):
        forms.add("k_run0")
    if nseg.max(initial=0) >= 2:
        forms.add("multi_seg")
    if count.max(initial=0) > 3:
        forms.add("slabs_gt3")
    return forms


def _check_balance(cus, ng, base, rem, n_tiles, skip, weights, sc, g, x, t, kb, ke, has_ex):
    """The cut of each slice's list, from the walk() budget.  Per slice: items of tile t cost w_t (1 on near-uniform lists, else the
    weight over the lightest tile's), a segment `sc` more.  ncx = max(1, min(cus / ng, items / 8)) workgroups may be used.  The greedy walk
    closes a workgroup only when the next segment of one item does not fit, i.e. above B - sc - w_max, so any budget
    B >= (W + (tiles + ncx) sc) / ncx + sc + w_max fits (segments <= tiles + one split per workgroup); the bisection's budget is below that,
    and a workgroup exceeds its budget only with a single one-item segment."""
    on = ~skip
    if not on.any():
        assert t.size == 0
        return
    w_min, w_max = weights[on].min(), weights[on].max()
    uniform = 4 * (w_max - w_min) < w_max
    wu = np.ones(n_tiles) if uniform else weights / max(w_min, 1.0)
    nk = (ke - kb) + has_ex
    load = np.bincount(g, weights=sc + nk * wu[t], minlength=cus)
    used = np.bincount(g, minlength=cus) > 0
    tix = np.arange(n_tiles)
    for xs in range(ng):
        cnt = base + (((xs - tix) % ng) < rem)
        L = int(cnt[on].sum())
        W = float((cnt * wu)[on].sum())
        ncx = max(1, min(cus // ng, L // 8))
        wg = np.flatnonzero((np.arange(cus) % 8) % ng == xs)
        assert used[wg].sum() <= ncx, (xs, used[wg].sum(), ncx)
        bound = max((W + (on.sum() + ncx) * sc) / ncx + sc + wu[on].max(), sc + wu[on].max())
        assert load[wg].max() <= bound * (1 + 1e-6), (xs, load[wg].max(), bound)


def _random_case(rng):
    cus = rng.choice([256, 248, 80, 8])
    ng = rng.choice([1, 2, 4, 8]) if cus % 8 == 0 else 1
    n_k = rng.choice([k for k in (65, 7, 130) if k >= ng])
    n_tiles_target = int(math.exp(rng.uniform(0, math.log(3000 if rng.random() < 0.05 else 400))))  # (few large lists: seconds, not minutes)
    shared = rng.random() < 0.4  # source row blocks: several tiles per destination chunk
    tiles, chunk, a0 = [], [], 0
    while len(tiles) < n_tiles_target:
        n = rng.choice([32, 32, rng.randint(1, 32), rng.randint(1, 8)])
        nb = rng.randint(2, 6) if shared and rng.random() < 0.5 else 1
        tiles += [(a0, n)] * nb  # (a chunk's tiles are adjacent, as plan_tiles emits them)
        chunk += [chunk[-1] + 1 if chunk else 0] * nb
        a0 += n
    kind = rng.choice(["uniform", "near", "wild", "span"])
    if kind == "uniform":
        w = [476 + 2 * 4] * len(tiles)
    elif kind == "near":
        w = [rng.randint(900, 1100) for _ in tiles]
    elif kind == "wild":
        w = [rng.choice([1, 10, 1000, rng.randint(1, 100000)]) for _ in tiles]
    else:  # the sampler's model: 476 + 2 (24 in dg_mode 1) per 16 source rows
        per = rng.choice([2, 24])
        w = [476 + per * ((rng.randint(1, 167) + 15) // 16) for _ in tiles]
    skip = None
    r = rng.random()
    if r < 0.3:
        p = rng.choice([0.05, 0.3, 0.9])
        skip = [1 if rng.random() < p else 0 for _ in tiles]
    elif r < 0.33:
        skip = [1] * len(tiles)
    seg_cost = rng.choice([0.0, 0.1, 3.6, 5.8, 100.0])
    return dict(cus=cus, ng=ng, n_k=n_k, n_atoms=a0, tiles=tiles, chunk=chunk, weights=w, skip=skip, seg_cost=seg_cost)


def _plan(case):
    from jamun_amd import native

    return native.plan_segments(case["cus"], case["ng"], case["n_k"], case["n_atoms"], case["tiles"], case["chunk"], case["weights"],
                                case["skip"], case["seg_cost"])


def _check(case, P):
    return check_plan(P["segs"], cus=case["cus"], ng=case["ng"], n_k=case["n_k"], n_atoms=case["n_atoms"], tiles=case["tiles"],
                      chunk=case["chunk"], max_segs=P["max_segs"], n_slabs=P["n_slabs"], atom_nslab=P["atom_nslab"], skip=case["skip"],
                      weights=case["weights"], seg_cost=case["seg_cost"])


def test_planner_fuzz_keeps_its_invariants_and_reaches_every_form():
    rng = random.Random(20261016)
    seen = {f: 0 for f in FORMS}
    n = 1500
    for i in range(n):
        case = _random_case(rng)
        P = _plan(case)
        try:
            forms = _check(case, P)
        except AssertionError as e:
            raise AssertionError(f"case {i}: cus={case['cus']} ng={case['ng']} n_k={case['n_k']} tiles={len(case['tiles'])} "
                                 f"seg_cost={case['seg_cost']}: {e}") from e
        for f in forms:
            seen[f] += 1
        if i % 10 == 0:  # deterministic: the same input plans the same lists
            Q = _plan(case)
            assert all(np.array_equal(P[k], Q[k]) for k in ("segs", "atom_nslab")) and P["n_slabs"] == Q["n_slabs"]
    print("plan forms seen over", n, "plans:", seen)
    assert all(seen[f] > 0 for f in FORMS), seen  # (the fuzz must not silently narrow)


@pytest.mark.parametrize("ng", [1, 2, 4, 8])
@pytest.mark.parametrize("seg_cost", [0.0, 3.6, 5.8])
def test_sampler_like_plans(ng, seg_cost):
    """The sampler's own inputs: 65 hidden units, 256 CUs, tiles of 32 destinations of the BASELINE molecule sizes."""
    for atoms, walkers in [(17, 64), (33, 64), (57, 32), (70, 16), (93, 8), (166, 4)]:
        tiles = []
        for wk in range(walkers):
            for d in range(0, atoms, 32):
                tiles.append((wk * atoms + d, min(32, atoms - d)))
        case = dict(cus=256, ng=ng, n_k=65, n_atoms=atoms * walkers, tiles=tiles, chunk=list(range(len(tiles))),
                    weights=[476 + 2 * ((atoms + 15) // 16)] * len(tiles), skip=None, seg_cost=seg_cost)
        forms = _check(case, _plan(case))
        if ng > 1:
            assert "k_extra" in forms  # (65 % ng == 1: every tile has one left-over unit)


def test_planner_rejects_what_the_sampler_never_asks_for():
    from jamun_amd import native

    with pytest.raises(RuntimeError, match="ng must be"):
        native.plan_segments(256, 3, 65, 32, [(0, 32)], [0], [1])
    with pytest.raises(RuntimeError, match="ng must be"):
        native.plan_segments(256, 8, 7, 32, [(0, 32)], [0], [1])
    with pytest.raises(RuntimeError, match="tile atoms"):
        native.plan_segments(256, 1, 65, 16, [(0, 32)], [0], [1])
    with pytest.raises(RuntimeError, match="weights"):
        native.plan_segments(256, 1, 65, 32, [(0, 32)], [0], [0])
