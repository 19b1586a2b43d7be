"""Records tests/golden/frames_refusals.json: what every bad call of tests/_refusal_cases.py answers, a return code and the library's error
text for a C entry, the exception class and its text for a Python entry point.  Recorded once, from the commit before the bindings moved
to jamun_amd/native_frames.py and came to share their checks; tests/test_frames_refusals_host.py holds every later tree to it, so it is not
to be recorded again from a tree under test.  Run from the repository root with the library built:

    python tests/golden/make_frames_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    import _refusal_cases as cases

    got = cases.answers()
    accepted = [name for name, a in got.items() if not a.get("code") and not a.get("raises")]
    if accepted:
        sys.exit(f"not refused: {accepted}")
    with open(os.path.join(HERE, "frames_refusals.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(name)}: {json.dumps(a)}" for name, a in got.items()) + "\n}\n")
