"""What encoding mels of different lengths in one call buys: 8 mels of 600 .. 752 latent tokens (1200 .. 1504 frames; the clip lengths of
tools/vae_lens_bench.py, all multiples of 4 tokens: one group of harness.plan_encode_calls), through the VAE encoder in three forms.

    lens    ONE call with row lengths (vb_vae_encode_lens), padded to the longest mel
    single  8 single-clip calls, one per mel at its own length (what a caller of encode_first_stage ran before)
    equal   the equal-length 8 x 752 call (vb_vae_encode: the lengths call does this much work, plus the mask, the table, the row-length forms
            of the statistics and the softmax, and one tail-zero launch per op that writes a raw activation buffer)

One process, one GPU, synthetic weights, the default encoder (384 / 768 / 1536 channels), per precision (fp32mf, split, bf16xt).  The encoder
calls alone are timed with HIP events on the pass's stream, --warmup passes per form first, then the forms alternated over --rounds rounds.
Reported: median and min .. max ms per pass of each form (a pass of `single` is its 8 calls), the two ratios and the number of tail-zero
launches per pass.  THE GATE: the lens call takes less time than the 8 single calls of the same run, in every precision - otherwise the
feature has no point and the tool exits 1.  The ratio to the equal-length call is recorded, not gated.  The forms are also checked against
each other: every row of the lens call equals its single call bit for bit on its valid columns and is zero behind them.

    python tools/vae_encode_lens_bench.py [--rounds 7] [--out profiles/vae_encode_lens_bench.json]
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
LENGTHS = (600, 624, 644, 668, 688, 708, 732, 752)      # latent tokens: the lengths of tools/vae_lens_bench.py
PRECISIONS = ("fp32mf", "split", "bf16xt")


def tail_zero_launches(net, L):
    """the ops net_run follows with a tail-zero launch under row lengths (versband_amd/csrc/convnet.hip)"""
    skip = (L.OP_XT_PLANES, L.OP_SPLIT_PLANES, L.OP_GN_STATS, L.OP_SOFTMAX_T)
    return sum(1 for op in net.nb.ops if op.kind not in skip and not (op.out >= 0 and net.nb.bufs[op.out][2] == 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 1
    if not torch.cuda.is_available():
        raise SystemExit("vae_encode_lens_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED
    from versband_amd import _lib as L
    from versband_amd import harness, synth
    from versband_amd.engine import Context, build_vae_encoder

    assert [c["rows"] for c in harness.plan_encode_calls(LENGTHS)] == [list(range(len(LENGTHS)))], "the lengths form one group"
    device = torch.device("cuda:0")
    B, T = len(LENGTHS), max(LENGTHS)
    vcfg = synth.VAEConfig()
    sd = synth.make_state_dict(synth.vae_encoder_shapes(vcfg), SEED + 3)
    ctx = Context(device)
    tm = 2 ** len(vcfg.down_layers)                       # mel frames per latent token
    z = torch.from_numpy(synth.prng.normal(5, B * vcfg.in_channels * T * tm).reshape(B, vcfg.in_channels, T * tm).copy()).float().to(device)
    clips = [z[b:b + 1, :, :n * tm].contiguous() for b, n in enumerate(LENGTHS)]
    stream = torch.cuda.Stream(device=device)
    res = {"workload": f"8 mels of {list(LENGTHS)} latent tokens ({2 * sum(LENGTHS) / 150.0:.1f} s of mel), VAE encoder (384 / 768 / 1536 channels), "
                       "encoder calls only", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_form": a.warmup,
           "padding_share": 1.0 - sum(LENGTHS) / (B * T), "precisions": {}}
    ok = True
    for prec in PRECISIONS:
        # one net per call shape: each keeps its own workspace
        net = {"lens": build_vae_encoder(ctx, sd, precision=prec), "equal": build_vae_encoder(ctx, sd, precision=prec),
               "single": [build_vae_encoder(ctx, sd, precision=prec) for _ in range(B)]}
        ms = {m: [] for m in FORMS}
        last = {}
        with torch.cuda.stream(stream):
            def one_pass(m):
                if m == "lens":
                    return net[m].encode_lens(z, list(LENGTHS))
                if m == "equal":
                    return net[m].run(z)
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
        rows_equal = all(bool(torch.equal(last["lens"][b, :, :n], last["single"][b][0])) for b, n in enumerate(LENGTHS))
        tails_zero = all(int(torch.count_nonzero(last["lens"][b, :, n:])) == 0 for b, n in enumerate(LENGTHS))
        gate = med["lens"] < med["single"]
        ok = ok and gate and rows_equal and tails_zero
        res["precisions"][prec] = {
            "median_ms_per_pass": med, "min_ms_per_pass": {m: min(ms[m]) for m in FORMS}, "max_ms_per_pass": {m: max(ms[m]) for m in FORMS},
            "ms_per_pass": ms, "lens_over_single": med["lens"] / med["single"], "lens_over_equal": med["lens"] / med["equal"],
            "tail_zero_launches_per_pass": tail_zero_launches(net["lens"], L), "ops_per_pass": len(net["lens"].nb.ops),
            "gate_lens_faster_than_single_calls": gate, "rows_equal_their_single_calls_bit_for_bit": rows_equal, "tails_are_exact_zeros": tails_zero}
        del net, last
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not ok:
        raise SystemExit("vae_encode_lens_bench: GATE FAILED - the lens call is not faster than the single calls, or its rows are not the single calls'")


if __name__ == "__main__":
    main()
