"""Writes tests/golden/decode_launches.json: (positions, launches, enc_rows, persistent) of
every decode call of tests/decode_launches.py (CASES), as the library built from the checked-out
commit runs them on the GPU. Recorded once, before the decode call's host side was split into
plan_decode / DecodeStep: a host-side change must reproduce it. Run from the repository root:
python tests/golden/make_decode_launches.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import decode_launches as dl  # noqa: E402


def main():
    engines, out = {}, {}
    for name, (model, _, _) in dl.CASES.items():     # in order: the staggered pair continues
        if model not in engines:
            engines[model] = dl.make_engine(model)
        out[name] = dl.run_case(engines[model], name)
        print(name, out[name], flush=True)
    with open(dl.golden_path(), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
