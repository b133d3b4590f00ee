"""What vocoding mels of different lengths in one BigVGAN call buys: 8 mels of 1200 .. 1504 frames (the clips of
tools/vocoder_lens_bench.py, all multiples of 4 frames: one group of harness.plan_vocoder_calls), through BigVGAN in three forms.

    lens    ONE call with row lengths (vb_bigvgan_forward_lens), padded to the longest mel
    single  8 single-clip calls, one per mel at its own length (all BigVGAN could do before)
    equal   the equal-length 8 x 1504 call (vb_hifigan_forward: the lengths call does this much work, plus the mask, the table and one
            tail-zero launch per op that is not an anti-aliased activation - those write their own zeros and skip the workgroups
            behind a row's end)

One process, one GPU, synthetic weights, the default generator (512 initial channels, hop 320), per precision (fp32mf, bf16xt).  The vocoder
calls alone are timed with HIP events on the pass's stream, --warmup passes per form first, then the forms alternated over --rounds rounds.
Reported: median and min .. max ms per pass of each form (a pass of `single` is its 8 calls), the two ratios and the number of tail-zero
launches per pass.  THE GATE: the lens call takes less time than the 8 single calls of the same run, in every precision - otherwise the
feature has no point and the tool exits 1.  The ratio to the equal-length call is recorded, not gated.  The forms are also checked against
each other: every row of the lens call equals its single call bit for bit on its valid samples and is zero behind them.

    python tools/bigvgan_lens_bench.py [--rounds 7] [--out profiles/bigvgan_lens_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

FORMS = ("lens", "single", "equal")
LENGTHS = (1200, 1248, 1288, 1336, 1376, 1416, 1464, 1504)      # mel frames: the clips of tools/vocoder_lens_bench.py
PRECISIONS = ("fp32mf", "bf16xt")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 1
    if not torch.cuda.is_available():
        raise SystemExit("bigvgan_lens_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED
    from versband_amd import _lib as L
    from versband_amd import harness, synth
    from versband_amd.engine import Context, build_bigvgan

    assert [c["rows"] for c in harness.plan_vocoder_calls(LENGTHS)] == [list(range(len(LENGTHS)))], "the lengths form one group"
    device = torch.device("cuda:0")
    B, T = len(LENGTHS), max(LENGTHS)
    hcfg = synth.BigVGANConfig()
    sd = synth.make_state_dict(synth.bigvgan_shapes(hcfg), SEED + 7)
    hop = math.prod(hcfg.upsample_rates)
    ctx = Context(device)
    mel = torch.from_numpy(synth.prng.uniform(5, B * 80 * T, -5.0, 1.5).reshape(B, 80, T).copy()).to(device)
    clips = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(LENGTHS)]
    stream = torch.cuda.Stream(device=device)
    res = {"workload": f"8 mels of {list(LENGTHS)} frames ({sum(LENGTHS) / 150.0:.1f} s of mel), BigVGAN (512 initial channels, hop {hop}), "
                       "vocoder calls only", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_form": a.warmup,
           "padding_share": 1.0 - sum(LENGTHS) / (B * T), "precisions": {}}
    ok = True
    for prec in PRECISIONS:
        # one net per call shape: each keeps its own workspace
        net = {"lens": build_bigvgan(ctx, sd, hcfg.as_hparams(), precision=prec), "equal": build_bigvgan(ctx, sd, hcfg.as_hparams(), precision=prec),
               "single": [build_bigvgan(ctx, sd, hcfg.as_hparams(), precision=prec) for _ in range(B)]}
        tail_launches = sum(1 for op in net["lens"].nb.ops if op.kind not in (L.OP_XT_PLANES, L.OP_AA_ACT))
        ms = {m: [] for m in FORMS}
        last = {}
        with torch.cuda.stream(stream):
            def one_pass(m):
                if m == "lens":
                    return net[m].vocode_lens(mel, list(LENGTHS))
                if m == "equal":
                    return net[m].run(mel)
                return [net[m][b].run(clips[b]) for b in range(B)]

            for m in FORMS:
                for _ in range(a.warmup):
                    w = one_pass(m)
                stream.synchronize()
                assert all(bool(torch.isfinite(t).all()) for t in (w if isinstance(w, list) else [w])), (prec, m)
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
        rows_equal = all(bool(torch.equal(last["lens"][b, :, :n * hop], last["single"][b][0])) for b, n in enumerate(LENGTHS))
        tails_zero = all(int(torch.count_nonzero(last["lens"][b, :, n * hop:])) == 0 for b, n in enumerate(LENGTHS))
        gate = med["lens"] < med["single"]
        ok = ok and gate and rows_equal and tails_zero
        res["precisions"][prec] = {
            "median_ms_per_pass": med, "min_ms_per_pass": {m: min(ms[m]) for m in FORMS}, "max_ms_per_pass": {m: max(ms[m]) for m in FORMS},
            "ms_per_pass": ms, "lens_over_single": med["lens"] / med["single"], "lens_over_equal": med["lens"] / med["equal"],
            "tail_zero_launches_per_pass": tail_launches, "ops_per_pass": len(net["lens"].nb.ops),
            "aa_act_ops_per_pass": sum(1 for op in net["lens"].nb.ops if op.kind == L.OP_AA_ACT),
            "gate_lens_faster_than_single_calls": gate, "rows_equal_their_single_calls_bit_for_bit": rows_equal, "tails_are_exact_zeros": tails_zero}
        del net, last
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not ok:
        raise SystemExit("bigvgan_lens_bench: GATE FAILED - the lens call is not faster than the single calls, or its rows are not the single calls'")


if __name__ == "__main__":
    main()
