"""What the band-limited resampler costs (janus_amd/audio.py, csrc/resample.hip, DESIGN.md
§5t): one JSON document on stdout and in --out (default profiles/resample.json).

Cases: one 600 s clip at 44.1 kHz, one 600 s clip at 48 kHz, 64 clips of 30 s at 44.1 kHz in
one call; seeded noise. Per case, after one warming call, three repeats of each row, reported
as min and max (host clock around a call that ends in a device synchronise):

  resampler_device_ms  Resampler on device tensors (input already on the device, output left
                       there): staging + kernel
  resampler_numpy_ms   Resampler on numpy arrays: the same plus both host copies
  to_16k_host_ms       the same input through common/wavio.py::to_16k on the host (np.interp;
                       x[::3] at 48 kHz)
  logmel_ms            WhisperEngine("tiny.en").logmel_frames of the resampled audio (device
                       in, device out), for scale

No threshold hangs on these numbers.

Usage (GPU box):  python tools/resample_bench.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
CASES = (("1x600s_44100", 1, 600, 44100), ("1x600s_48000", 1, 600, 48000), ("64x30s_44100", 64, 30, 44100))


def timed(f):
    import torch
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"min": round(min(out), 3), "max": round(max(out), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from janus_amd.audio import Resampler
    from janus_amd.common.wavio import to_16k
    from janus_amd.whisper import CONFIGS, WhisperEngine
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(CONFIGS["tiny.en"])
    doc = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "cases": {}}
    for name, n_clips, seconds, sr in CASES:
        rng = np.random.default_rng(sr + n_clips)
        clips = [(rng.normal(size=seconds * sr) * 0.1).astype(np.float32) for _ in range(n_clips)]
        r = Resampler(sr, 16000, dev)
        on_dev = [torch.from_numpy(c).to(dev) for c in clips]
        out = r(on_dev)   # warms; grows the staging buffer once
        torch.cuda.synchronize()
        n_out = [int(o.shape[0]) for o in out]
        pcm = torch.cat(list(out) + [torch.zeros(1, device=dev)])
        offs = torch.tensor(np.concatenate([[0], np.cumsum(n_out)]), dtype=torch.int64, device=dev)
        frames = n_out[0] // 160
        eng.logmel_frames(pcm, offs, n_clips, 1, frames)
        torch.cuda.synchronize()
        row = {"clips": n_clips, "seconds": seconds, "sr_in": sr, "L": r.L, "M": r.M, "taps": r.T,
               "samples_in": int(sum(len(c) for c in clips)), "samples_out": int(sum(n_out)),
               "resampler_device_ms": timed(lambda: r(on_dev)),
               "resampler_numpy_ms": timed(lambda: r(clips)),
               "to_16k_host_ms": timed(lambda: [to_16k(c, sr) for c in clips]),
               "logmel_ms": timed(lambda: eng.logmel_frames(pcm, offs, n_clips, 1, frames))}
        doc["cases"][name] = row
        print(name, json.dumps(row), flush=True)
        del r, on_dev, out, pcm
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
