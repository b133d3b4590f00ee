"""What analysing waveforms of different lengths in one MelNet call buys: 8 waveforms of 1200 .. 1504 frames x 320 samples (the vocoded clips
of tools/vocoder_lens_bench.py) through the log-mel front-end in three forms, each as the mel alone and as the mel with the masked distance
against a decoded mel (the two steps of scripts/infer_batched.py --eval_mel).

    lens    ONE call with row lengths (vb_melnet_forward_lens), padded to the longest waveform; with the distance: + ONE vb_mel_dist_lens call
    single  8 single-clip calls, one per waveform at its own length (the per-clip path); with the distance: + 8 one-row vb_mel_dist_lens calls
    equal   the equal-length 8 x 1504-frame call (vb_melnet_forward: the lengths call does this much work, plus two tables and the tail pass
            over the spectrum); with the distance: + ONE vb_mel_dist_lens call over full rows

One process, one GPU.  Inputs are on the device before the clock starts: the calls alone are timed, with HIP events on the pass's stream.  A
call takes tens of microseconds, so a timed window is --iters passes of one form (a pass of `single` is its 8 calls) and the figure is the
window over --iters; every form is warmed up first and the forms are alternated over --rounds rounds.  Reported: median and min .. max
microseconds per pass, and the ratios.  NOTHING IS GATED: nobody had measured these, the tool records what comes out.  The forms are checked
against each other: every row of the lens call equals its single call bit for bit on its frames and is zero behind them, and so do the distances.

    python tools/melnet_lens_bench.py [--rounds 7] [--iters 50] [--out profiles/melnet_lens_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FORMS = ("lens", "single", "equal")
STEPS = ("mel", "mel+dist")
FRAMES = (1200, 1248, 1288, 1336, 1376, 1416, 1464, 1504)      # the mel lengths of tools/vocoder_lens_bench.py
HOP = 320
MEL_HP = dict(fft_size=1280, audio_num_mel_bins=80, audio_sample_rate=24000, hop_size=HOP, win_size=1280, fmin=0, fmax=8000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="passes per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the result (raw per-window figures included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.iters >= 1 and a.warmup >= 1
    if not torch.cuda.is_available():
        raise SystemExit("melnet_lens_bench: no GPU - this is a measurement, there is nothing to report without one")

    from versband_amd import synth
    from versband_amd.melnet import MelNet, mel_distance

    device = torch.device("cuda:0")
    B, T = len(FRAMES), max(FRAMES)
    lens = [f * HOP for f in FRAMES]
    wav = torch.from_numpy(synth.prng.uniform(5, B * T * HOP, -1.1, 1.1).reshape(B, T * HOP).copy()).to(device)
    dec = torch.from_numpy(synth.prng.uniform(6, B * 80 * T, -5.0, 0.5).reshape(B, 80, T).copy()).to(device)
    clips = [wav[b, :n].contiguous() for b, n in enumerate(lens)]
    decs = [dec[b:b + 1, :, :f].contiguous() for b, f in enumerate(FRAMES)]
    # one front-end per call shape: each keeps its own workspace
    net = {"lens": MelNet(MEL_HP, device=device), "equal": MelNet(MEL_HP, device=device), "single": [MelNet(MEL_HP, device=device) for _ in range(B)]}
    stream = torch.cuda.Stream(device=device)

    def one_pass(form, step):
        if form == "single":
            mels = [net[form][b](clips[b]) for b in range(B)]
            return mels, ([mel_distance(mels[b], decs[b], [FRAMES[b]], remove_offset=True) for b in range(B)] if step == "mel+dist" else None)
        mel = net[form](wav, lengths=lens) if form == "lens" else net[form](wav)
        frames = list(FRAMES) if form == "lens" else [T] * B
        return mel, (mel_distance(mel, dec, frames, remove_offset=True) if step == "mel+dist" else None)

    us = {s: {m: [] for m in FORMS} for s in STEPS}
    last = {}
    with torch.cuda.stream(stream):
        for s in STEPS:
            for m in FORMS:
                for _ in range(a.warmup):
                    one_pass(m, s)
        stream.synchronize()
        for r in range(a.rounds):
            for s in STEPS:
                for m in FORMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.iters):
                        last[(m, s)] = one_pass(m, s)
                    e1.record(stream)
                    e1.synchronize()
                    us[s][m].append(1000.0 * e0.elapsed_time(e1) / a.iters)
            print(f"round {r}: " + "   ".join(f"{s}: " + " ".join(f"{m} {us[s][m][-1]:.1f}" for m in FORMS) for s in STEPS) + "  (us per pass)", flush=True)
    mel_l, (dist_l, off_l) = last[("lens", "mel+dist")]
    mels_s, dists_s = last[("single", "mel+dist")]
    rows_equal = all(bool(torch.equal(mel_l[b, :, :f], mels_s[b][0])) for b, f in enumerate(FRAMES))
    tails_zero = all(int(torch.count_nonzero(mel_l[b, :, f:])) == 0 for b, f in enumerate(FRAMES))
    dists_equal = all(bool(torch.equal(dist_l[b:b + 1], dists_s[b][0])) and bool(torch.equal(off_l[b:b + 1], dists_s[b][1])) for b in range(B))
    res = {"workload": f"8 waveforms of {list(FRAMES)} frames x {HOP} samples ({sum(FRAMES) / 75.0:.1f} s of audio at 24 kHz), MelNet (n_fft 1280, hop 320, 80 mels); "
                       "mel+dist adds the masked distance against a decoded mel with the offset removed; inputs on the device, calls only",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "passes_per_timed_window": a.iters, "warmup_passes_per_form": a.warmup,
           "padding_share": 1.0 - sum(FRAMES) / (B * T), "steps": {},
           "rows_equal_their_single_calls_bit_for_bit": rows_equal, "tails_are_exact_zeros": tails_zero, "distances_equal_their_single_calls_bit_for_bit": dists_equal}
    for s in STEPS:
        med = {m: statistics.median(us[s][m]) for m in FORMS}
        res["steps"][s] = {"median_us_per_pass": med, "min_us_per_pass": {m: min(us[s][m]) for m in FORMS}, "max_us_per_pass": {m: max(us[s][m]) for m in FORMS},
                           "us_per_pass": us[s], "lens_over_single": med["lens"] / med["single"], "lens_over_equal": med["lens"] / med["equal"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not (rows_equal and tails_zero and dists_equal):
        raise SystemExit("melnet_lens_bench: the lens call's rows are not the single calls'")


if __name__ == "__main__":
    main()
