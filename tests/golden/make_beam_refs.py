"""Writes tests/golden/beam_refs.json: the reference results of the beam decode cases of
tests/beam_ref.py (CASES, TRANSCRIBE_CASE), computed on the CPU by tests/beam_ref.py over
the oracle. Run from the repository root: python tests/golden/make_beam_refs.py [case ...]
(no argument: every case; named cases replace their entries only)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import beam_ref  # noqa: E402
from janus_amd import tokenizer as tok  # noqa: E402


def main(names):
    tk = tok.load_tokenizer()
    out = beam_ref._golden()
    for name in names or list(beam_ref.CASES) + ["transcribe"]:
        if name == "transcribe":
            out[name] = dict(case=beam_ref.TRANSCRIBE_CASE, **beam_ref.compute_transcribe(tk))
        else:
            out[name] = dict(case=beam_ref.CASES[name], windows=beam_ref.compute_case(name, tk))
        print(name, "done", flush=True)
        with open(beam_ref.golden_path(), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
