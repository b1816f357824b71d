"""Writes tests/golden/plan_descriptions.json: janus_decode_plan_describe's text and graph
key for the planner calls of tests/multilingual_ref.py PLAN_CASES, as the commit BEFORE
janus_decode_rows.no_speech_back printed them (run on that commit; the struct then ends at
`steps`, which the trailing field of a newer ctypes mirror does not disturb). The multilingual
host test holds a plan with no_speech_back 0 to these, the new field's own line and key word
aside. Usage: python tests/golden/make_plan_descriptions.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import multilingual_ref as mr  # noqa: E402
from janus_amd import _native as nat  # noqa: E402


def main():
    lib = nat.lib()
    out = {}
    for name in mr.PLAN_CASES:
        text, key = mr.describe_plan(lib, name)
        out[name] = {"text": text, "key": list(key)}
    with open(os.path.join(HERE, "plan_descriptions.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
