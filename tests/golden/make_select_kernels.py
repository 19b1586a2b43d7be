"""Records tests/golden/select_kernels.json: for every case of ``_select_cases.golden_inputs`` the inputs as parameters, the output array
of ``jamun_debug_select_kernels`` and a CRC of each list it returns.  Run from the repository root with the library built:

    python tests/golden/make_select_kernels.py
"""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def record(case):
    import _select_cases as sel
    from jamun_amd import native

    r = sel.golden_select(case)
    return dict(case, out=[r[k] for k in native.SELECT_KEYS], crc={k: zlib.crc32(r[k].tobytes()) for k in native.SELECT_LISTS})


if __name__ == "__main__":
    import _select_cases as sel

    with open(os.path.join(HERE, "select_kernels.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(record(c)) for c in sel.golden_inputs()) + "\n]\n")
