"""What vocoding long mels of different lengths in one chunked call costs: 4 mels of 3600 / 4400 / 5200 / 6000 frames (24 .. 40 s; all
multiples of 4 frames: one group of harness.plan_vocoder_calls), chunk = 3000, halo = 32, through the HiFi-GAN in three forms.

    lens    ONE chunked call with row lengths (vb_hifigan_forward_chunked_lens), padded to the longest mel
    single  4 single-clip chunked calls (vb_hifigan_forward_chunked), one per mel at its own length
    equal   the equal-length 4 x 6000 chunked call (vb_hifigan_forward_chunked: what vocoding the zero-padded batch costs)

One process, one GPU, synthetic weights, the default generator (512 initial channels, hop 320), per precision (fp32mf, bf16xt).  The vocoder
calls alone are timed with HIP events on the pass's stream, --warmup passes per form first, then the forms alternated over --rounds rounds.
Reported: median and min .. max ms per pass of each form (a pass of `single` is its 4 calls), the ratios, the frames each form runs the
generator on (harness.plan_chunk_calls: the lens call runs every active row of a chunk at the chunk's width), and THE SPREAD of the single
calls from round to round ((max - min) / median).  The expectation recorded, not gated: the lens call takes no longer than the 4 single
calls by more than that spread.  What is gated (exit 1): every row of the lens call equals its single call bit for bit on its own samples
and is zero behind them.

    python tools/vocoder_chunked_lens_bench.py [--rounds 7] [--out profiles/vocoder_chunked_lens_bench.json]
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
LENGTHS = (3600, 4400, 5200, 6000)      # mel frames
CHUNK, HALO = 3000, 32
PRECISIONS = ("fp32mf", "bf16xt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 1
    if not torch.cuda.is_available():
        raise SystemExit("vocoder_chunked_lens_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED
    from versband_amd import harness, synth
    from versband_amd.engine import Context, build_hifigan

    assert [c["rows"] for c in harness.plan_vocoder_calls(LENGTHS)] == [list(range(len(LENGTHS)))], "the lengths form one group"
    device = torch.device("cuda:0")
    B, T = len(LENGTHS), max(LENGTHS)
    steps = harness.plan_chunk_calls(LENGTHS, T, CHUNK, HALO)
    assert all(n % 4 == c["tc"] % 4 for c in steps for n in c["n"]), "every chunk keeps the residue: rows are bit-equal to the clip alone"
    frames = {"lens": sum(len(c["rows"]) * c["tc"] for c in steps),
              "single": sum(c["tc"] for n in LENGTHS for c in harness.plan_chunk_calls([n], n, CHUNK, HALO)),
              "equal": sum(B * c["tc"] for c in harness.plan_chunk_calls([T] * B, T, CHUNK, HALO))}
    hcfg = synth.HifiGanConfig()
    hop = hcfg.hop
    sd = synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2)
    ctx = Context(device)
    mel = torch.from_numpy(synth.prng.uniform(5, B * 80 * T, -5.0, 1.5).reshape(B, 80, T).copy()).to(device)
    clips = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENGTHS)]
    stream = torch.cuda.Stream(device=device)
    res = {"workload": f"4 mels of {list(LENGTHS)} frames ({sum(LENGTHS) / 150.0:.1f} s of mel), chunk {CHUNK}, halo {HALO}, HiFi-GAN (512 initial "
                       f"channels, hop {hop}), vocoder calls only", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "warmup_passes_per_form": a.warmup, "padding_share": 1.0 - sum(LENGTHS) / (B * T), "generator_frames_per_pass": frames,
           "chunks": [{k: c[k] for k in ("s", "lo", "tc", "rows", "n")} for c in steps], "precisions": {}}
    ok = True
    for prec in PRECISIONS:
        # one net per call shape: each keeps its own workspace and scratch
        net = {"lens": build_hifigan(ctx, sd, hcfg.as_hparams(), precision=prec), "equal": build_hifigan(ctx, sd, hcfg.as_hparams(), precision=prec),
               "single": [build_hifigan(ctx, sd, hcfg.as_hparams(), precision=prec) for _ in range(B)]}
        ms = {m: [] for m in FORMS}
        last = {}
        with torch.cuda.stream(stream):
            def one_pass(m):
                if m == "lens":
                    return net[m].run_chunked(mel, CHUNK, HALO, lengths=list(LENGTHS))
                if m == "equal":
                    return net[m].run_chunked(mel, CHUNK, HALO)
                return [net[m][b].run_chunked(clips[b], CHUNK, HALO) for b in range(B)]

            for m in FORMS:
                for _ in range(a.warmup):
                    w = one_pass(m)
                stream.synchronize()
                assert all(bool(torch.isfinite(t).all()) for t in (w if isinstance(w, list) else [w])), (prec, m)
                del w
            for r in range(a.rounds):
                for m in FORMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    last[m] = one_pass(m)
                    e1.record(stream)
                    e1.synchronize()
                    ms[m].append(e0.elapsed_time(e1))
                print(f"[{prec}] round {r}: " + "  ".join(f"{m} {ms[m][-1]:.2f} ms" for m in FORMS), flush=True)
        med = {m: statistics.median(ms[m]) for m in FORMS}
        spread = {m: (max(ms[m]) - min(ms[m])) / med[m] for m in FORMS}
        rows_equal = all(bool(torch.equal(last["lens"][b, :, :n * hop], last["single"][b][0])) for b, n in enumerate(LENGTHS))
        tails_zero = all(int(torch.count_nonzero(last["lens"][b, :, n * hop:])) == 0 for b, n in enumerate(LENGTHS))
        held = med["lens"] <= med["single"] * (1.0 + spread["single"])
        print(f"[{prec}] median ms: " + "  ".join(f"{m} {med[m]:.2f}" for m in FORMS) + f"; spread of the single calls {100 * spread['single']:.1f} %; "
              f"lens / single {med['lens'] / med['single']:.3f}, lens / equal {med['lens'] / med['equal']:.3f}; the lens call is "
              + ("no slower than the single calls beyond their spread" if held else "SLOWER than the single calls by more than their spread"), flush=True)
        ok = ok and rows_equal and tails_zero
        res["precisions"][prec] = {
            "median_ms_per_pass": med, "min_ms_per_pass": {m: min(ms[m]) for m in FORMS}, "max_ms_per_pass": {m: max(ms[m]) for m in FORMS},
            "round_to_round_spread": spread, "ms_per_pass": ms, "lens_over_single": med["lens"] / med["single"],
            "lens_over_equal": med["lens"] / med["equal"], "lens_no_slower_than_single_calls_beyond_their_spread": held,
            "rows_equal_their_single_calls_bit_for_bit": rows_equal, "tails_are_exact_zeros": tails_zero}
        del net, last
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not ok:
        raise SystemExit("vocoder_chunked_lens_bench: FAILED - a row of the lens call is not its single call's, or has samples behind its end")


if __name__ == "__main__":
    main()
