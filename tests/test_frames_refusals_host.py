"""CPU tests: every refusal of the frame-analysis bindings that ends before a GPU is needed, the C entries of csrc/jamun_frames.cpp and the
Python entry points of jamun_amd/native_frames.py alike, is answered as tests/golden/frames_refusals.json records it (the same code or
exception class, the same text, the same one of two faults), and no entry is without a case.  The cases are tests/_refusal_cases.py's."""
import inspect
import json
import os
import re

import pytest

import _refusal_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "frames_refusals.json")))


@pytest.fixture(scope="module")
def lib():
    from jamun_amd import _lib

    return _lib.load()


def test_the_record_holds_the_cases_of_the_table_and_only_refusals(recorded):
    assert list(recorded) == list(cases.C_CASES) + list(cases.PY_CASES)
    assert all(a.get("code") or a.get("raises") for a in recorded.values())


@pytest.mark.parametrize("name", list(cases.C_CASES))
def test_c_entry_refuses_as_recorded(name, lib, recorded):
    entry, args = cases.C_CASES[name]
    assert cases.c_answer(lib, entry, args) == recorded[name]


@pytest.mark.parametrize("name", list(cases.PY_CASES))
def test_python_entry_refuses_as_recorded(name, recorded):
    from jamun_amd import native

    fn, make = cases.PY_CASES[name]
    assert cases.py_answer(native, fn, make) == recorded[name]


def test_state_map_takes_the_host_tables_it_always_took():
    """What `_state_map` accepts is no refusal, so the record cannot hold it: a host table of any number type is converted to int32 (floats
    are cut off towards zero), a scalar is a table of one entry, no map leaves the states as the labels; an int32 tensor is used as it is."""
    import numpy as np
    import torch

    from jamun_amd import native

    for given, want in ((5, [5]), (np.int32(3), [3]), ([0, 2, -1], [0, 2, -1]), ([0.0, 1.9, -1.0], [0, 1, -1]), (np.arange(4, dtype=np.int64), [0, 1, 2, 3]),
                        (torch.tensor([1, 0], dtype=torch.int32), [1, 0]), (np.array([1, 0], dtype=np.uint8), [1, 0])):
        table, n_in = native._state_map(given, 4, torch.device("cpu"))
        assert table.dtype == torch.int32 and table.is_contiguous() and table.tolist() == want and n_in == len(want), given
    assert native._state_map(None, np.int64(7), torch.device("cpu")) == (None, 7)


def test_every_c_entry_has_a_case_with_one_fault_and_one_with_two():
    """The entries are those of `_lib.SYMBOLS` that csrc/jamun_frames.cpp defines.  Each has its null-argument refusal and a case of two
    faults ("a_then_b"); no case passes an address where the entry requires a device pointer."""
    from jamun_amd import _lib

    src = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_frames.cpp")).read()
    entries = [n for n in _lib.SYMBOLS if re.search(rf"^int {n}\(", src, flags=re.M)]
    assert len(entries) >= 24 and set(entries) == set(cases.C_ENTRIES)
    for entry in entries:
        names = [n.split("/")[1] for n, (e, _) in cases.C_CASES.items() if e == entry]
        assert "null" in names and any("_then_" in n for n in names), entry
        assert len(cases.C_ENTRIES[entry]) == len(_lib.SYMBOLS[entry][1]), entry
    optional = {"prev_labels_dev", "n_changed_dev", "map_dev"}
    for name, (entry, args) in cases.C_CASES.items():
        for arg, a in zip(cases.C_ENTRIES[entry], args):
            assert a != cases.HOST or arg in optional, name
            assert not arg.endswith("_dev") or a in (None, cases.HOST), name


def test_every_python_entry_that_takes_a_tensor_has_a_case():
    """The entry points are the public functions jamun_amd/native_frames.py defines with a parameter that is a tensor or a table that may be
    one (annotated ``torch.Tensor``, or left without an annotation); `jamun_amd.native` hands out the same objects."""
    from jamun_amd import native, native_frames

    def takes_tensor(f):
        return any(p.annotation is inspect.Parameter.empty or "Tensor" in str(p.annotation) for p in inspect.signature(f).parameters.values())

    public = [n for n, f in vars(native_frames).items() if inspect.isfunction(f) and f.__module__ == native_frames.__name__ and not n.startswith("_")]
    entries = [n for n in public if takes_tensor(getattr(native_frames, n))]
    assert len(entries) >= 24
    covered = {fn for fn, _ in cases.PY_CASES.values()}
    assert not [n for n in entries if n not in covered]
    assert all(getattr(native, n) is getattr(native_frames, n) for n in public)
