"""Writes tests/golden/history_refs.json: the reference decodes of tests/history_ref.py (the
history rules in numpy over the unchanged oracle) for every model and option set of its SEEDS,
and the reference seek loop of its TRANSCRIBE_CASE. CPU only, a few minutes.

For every decode case it asserts (history_ref.check_case) that each row's smallest top-2
margin of the penalised keys is >= 2 NEAR_TIE — so the GPU tests may demand identical tokens at
every position — that each form differs from the same decode without options, and that the
row whose prompt holds a token it samples depends on the prompt staying out of the history.
Usage: python tests/golden/make_history_refs.py [case ...]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import history_ref as hr  # noqa: E402


def main(only):
    out = hr._golden()
    for model in hr.MODELS:
        for p, n in hr.OPTION_SETS:
            name = hr.case_name(model, p, n)
            if (only and name not in only) or name not in hr.SEEDS:
                continue
            c = hr.compute_case(model, p, n)
            hr.check_case(c, p)
            out[name] = c
            print(name, "smallest margin", min(r["min_margin"] for f in ("greedy", "prompt", "sampled") for r in c[f]))
    if not only or "transcribe" in only:
        tk = hr.tokenizer_for(hr.model_cfg("tiny"))
        t = hr.compute_transcribe(tk)
        t["plain_segments"] = hr.compute_transcribe(tk, options=False)["segments"]
        t["case"] = hr.TRANSCRIBE_CASE
        assert len(t["windows"]) >= 2
        assert min(w["min_margin"] for w in t["windows"]) >= hr.MIN_MARGIN, [w["min_margin"] for w in t["windows"]]
        assert [g[2] for g in t["segments"]] != [g[2] for g in t["plain_segments"]]
        # the options show in the prompts: <|startofprev|> and the hotwords open every window's
        for w in t["windows"]:
            assert w["prompt"][1:1 + len(hr.TRANSCRIBE_CASE["hotwords"])] == hr.TRANSCRIBE_CASE["hotwords"]
        out["transcribe"] = t
        print("transcribe", [w["min_margin"] for w in t["windows"]])
    with open(hr.golden_path(), "w") as f:
        json.dump(out, f, indent=None, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(set(sys.argv[1:]))
