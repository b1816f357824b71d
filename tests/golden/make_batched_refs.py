"""Writes tests/golden/batched_refs.json: the oracle's greedy decode (with timestamps) of every
chunk of tests/batched_ref.py's PARITY_CASE as a 30 s window of its own, and the segments
sliced from the chunk's start. CPU only, under a minute.

It asserts that every chunk's smallest top-2 margin is >= 2 NEAR_TIE, so the GPU test may
demand identical tokens at every position of every chunk, and that the chunks' decodes
differ (in tokens for some, in their statistics for all).
Usage: python tests/golden/make_batched_refs.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import batched_ref as br  # noqa: E402


def main():
    ref = br.compute_parity()
    margins = [c["min_margin"] for c in ref["chunks"]]
    print("smallest margins per chunk", margins)
    assert min(margins) >= br.MIN_MARGIN, margins
    # (seeded weights follow the audio weakly: short chunks may decode alike; the statistics differ)
    toks = [tuple(c["tokens"]) for c in ref["chunks"]]
    print("distinct decodes", len(set(toks)), "of", len(toks))
    assert len(set(toks)) >= 2 and all(toks), "every chunk decodes alike, or one to nothing"
    assert len({c["avg"] for c in ref["chunks"]}) == len(toks)
    assert len(ref["segments"]) >= len(ref["chunks"]) - 1
    assert ref["segments"][0][0] >= ref["chunks"][0]["start"] / 16000.0
    with open(br.golden_path(), "w") as f:
        json.dump(ref, f, indent=None, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
