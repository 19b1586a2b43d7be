"""CPU tests: the kernel selection of jamun_sampler_create (``select_kernels`` in jamun_plan.cpp, reached through
``jamun_debug_select_kernels``).  Three parts: the selections the GPU tests assert on ``jamun_sampler_stats``, asked on the CPU from the same
table (``_select_cases.py``); a golden of the full output over a case list that reaches every branch of the selection, recorded before the
selection was split into stages and the sampler came to hold its plan; and the planner's invariants (``check_plan`` of test_plan.py) on
every work list the selection emits."""
import json
import os
import zlib

import numpy as np
import pytest

import _select_cases as sel
from test_plan import check_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_kernels.json")
ANCHORS = sel.anchors()


@pytest.mark.parametrize("name,kind,arch,tuning,stats_ok", ANCHORS, ids=[a[0] for a in ANCHORS])
def test_host_selection_gives_what_the_gpu_tests_expect_of_the_stats(name, kind, arch, tuning, stats_ok):
    mols = sel.molecules(kind)
    r = sel.select(mols, arch, tuning)
    st = sel.as_stats(r)
    assert stats_ok(st), (name, st)
    assert st["edge_stride"] == sel.sp.edge_stride(mols)
    if arch == "conv" and not tuning and st["dg_mode"] == 4:  # (the rule test_gpu_switches.py restates: k_conv_mfi up to 32 distinct rows)
        assert st["init_path"] == sel.sc.expected_init_path(mols, False)


def _cases():
    from jamun_amd import native

    cases = json.load(open(GOLDEN))
    return cases, [dict(zip(native.SELECT_KEYS, c["out"])) for c in cases]


def test_golden_case_list_is_the_generated_one_and_reaches_every_branch():
    cases, outs = _cases()
    inputs = [{k: v for k, v in c.items() if k not in ("out", "crc")} for c in cases]
    assert inputs == json.loads(json.dumps(sel.golden_inputs()))
    dg = [o for o in outs if o["conv_path"] == 2]
    reached = lambda key, values, among=outs: {o[key] for o in among} >= set(values)
    assert reached("dg_mode", range(6), dg)
    assert reached("init_path", (0, 2, 3, 4, 5, 6, -1))
    assert reached("conv_path", (0, 2, 3, -1))
    assert reached("row_blocks", (0, 1), dg)
    assert any(o["n_tail_tiles"] > 0 for o in dg) and any(o["n_tail_tiles"] == 0 and o["dg_mode"] == 4 for o in dg)
    assert reached("init_tail", (0, 1), dg) and reached("own_init_segs", (0, 1), dg)
    assert reached("mf_nks", (3, 4), [o for o in dg if o["dg_mode"] == 4])
    assert reached("ml_window", (96, 128, 168), [o for o in dg if o["dg_mode"] == 5])
    assert reached("initv_nbuf", (1, 2), [o for o in dg if o["init_path"] == 2])
    assert any(o["ng"] > 1 for o in dg) and reached("dg_emu", (0, 1), dg)


def test_selection_matches_the_golden_and_its_work_lists_keep_the_planner_invariants():
    from jamun_amd import native

    cases, outs = _cases()
    for i, (c, want) in enumerate(zip(cases, outs)):
        r = sel.golden_select(c)
        got = {k: r[k] for k in native.SELECT_KEYS}
        assert got == want, (i, c["sizes"][:4], c["tuning"], {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        assert {k: zlib.crc32(r[k].tobytes()) for k in native.SELECT_LISTS} == c["crc"], (i, "a work list or tile table changed")
        if r["conv_path"] != 2:
            assert all(r[k].size == 0 for k in ("segs", "init_segs", "tail_tiles", "tiles", "chunk"))
            continue
        n_atoms, n_k = int(sum(c["sizes"])), sel.hparams(c["arch"])["edge_attr_dim"] + 1
        tiles, spans = r["tiles"][:, :2], r["tiles"][:, 2:]
        assert r["n_tiles"] == len(tiles) and r["span_max"] == int((spans[:, 1] - spans[:, 0]).max())
        tt = r["tail_tiles"]  # {first tail destination, first atom, atoms | source rows << 8, first source row}: the tile's descriptor
        skip = np.isin(tiles[:, 0], tt[:, 1])  # (no source row blocks beside tail tiles: a first atom names one tile)
        assert int(skip.sum()) == r["n_tail_tiles"] == len(tt) and int(tiles[skip, 1].sum()) == r["n_tail"]
        assert np.array_equal(tt[:, 2], tiles[skip, 1] | ((spans[skip, 1] - spans[skip, 0]) << 8)) and np.array_equal(tt[:, 3], spans[skip, 0])
        assert np.array_equal(tt[:, 0], np.cumsum(tiles[skip, 1]) - tiles[skip, 1]) and (not skip.any() or tiles[skip, 1].max() <= 8)
        weights = 476 + (24 if r["dg_mode"] == 1 else 2) * ((spans[:, 1] - spans[:, 0] + 15) // 16)  # (test_gpu_plans.py: the sampler's tile weights)
        common = dict(cus=c["cus"], ng=r["ng"], n_k=n_k, n_atoms=n_atoms, tiles=tiles, chunk=r["chunk"], weights=weights, seg_cost=r["seg_cost_tenths"] / 10)
        try:
            check_plan(r["segs"], max_segs=r["max_segs"], n_slabs=r["n_slabs"], atom_nslab=r["atom_nslab"], skip=skip if skip.any() else None,
                       skipped_nslab=r["tail_runs"] if skip.any() else None, **common)
            assert (r["init_segs"].size > 0) == bool(r["own_init_segs"])
            if r["own_init_segs"]:  # the initial projector's own lists: every tile, the tail tiles included
                check_plan(r["init_segs"], max_segs=r["init_max_segs"], n_slabs=r["init_n_slabs"], atom_nslab=r["init_atom_nslab"], **common)
        except AssertionError as e:
            raise AssertionError(f"case {i}: sizes={c['sizes'][:4]}.. tuning={c['tuning']} cus={c['cus']}: {e}") from e
