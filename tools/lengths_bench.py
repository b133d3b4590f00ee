"""What batching clips of different lengths buys: 8 clips at lengths spread over [600, 752] latent tokens, sampled in three forms.

    lens    ONE call with row lengths (vb_sample_cfg_lens), padded to the longest clip
    single  8 single-clip calls, one per clip at its own length (what a manifest of mixed lengths ran as before)
    equal   the equal-length 8 x 752 call (the upper yardstick: the lengths call does this much work, plus the table)

One process, one GPU: 50 Euler steps, bf16 DiT, synthetic weights.  The sampler calls alone are timed (the conditioning is precomputed
once per form, outside the timing), graph replay, with HIP events on the pass's stream, two warm-up passes per form (the second captures
the step loop's graph), then the forms alternated over --rounds rounds.  Reported: median and min .. max ms per pass of each form (a pass
of `single` is its 8 calls) and the two ratios.  There is no gate.  The forms are also checked against each other: every row of the
lengths call equals its single call bit for bit on the valid tokens.

    python tools/lengths_bench.py [--rounds 7] [--out profiles/lengths_bench.json]
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
LENGTHS = (600, 624, 644, 668, 688, 708, 732, 752)      # latent tokens: 16.0 .. 20.1 s, every one a multiple of 8 mel frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flow-steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 2, "the second warm-up pass captures the graph"
    if not torch.cuda.is_available():
        raise SystemExit("lengths_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED
    from versband_amd import model as vm
    from versband_amd import synth
    from versband_amd.engine import Context, DiTEngine

    device = torch.device("cuda:0")
    B, T, Lc = len(LENGTHS), max(LENGTHS), 80
    dcfg = synth.DiTConfig()
    ctx = Context(device)
    sd = synth.make_state_dict(synth.dit_shapes(dcfg), SEED)
    base = DiTEngine(ctx, dcfg, sd, precision="bf16")
    # one engine handle per call shape (shared packed weights): each keeps its own buffers and graph cache
    eng = {"lens": base, "equal": DiTEngine(ctx, dcfg, sd, precision="bf16", share=base),
           "single": [DiTEngine(ctx, dcfg, sd, precision="bf16", share=base) for _ in range(B)]}
    clips = [{k: v.to(device) for k, v in synth.make_clip_inputs(SEED, b, n, L=Lc).items()} for b, n in enumerate(LENGTHS)]
    full = [{k: v.to(device) for k, v in synth.make_clip_inputs(SEED, b, T, L=Lc).items()} for b in range(B)]
    x = torch.zeros(B, dcfg.in_channels, T, device=device)
    midi, beats = torch.zeros(B, 2 * T, dtype=torch.int64, device=device), torch.zeros(B, 2 * T, dtype=torch.int64, device=device)
    for b, (c, n) in enumerate(zip(clips, LENGTHS)):
        x[b, :, :n], midi[b, :2 * n], beats[b, :2 * n] = c["x_latent"], c["midi"].reshape(-1), c["beats"].reshape(-1)
    t5 = torch.cat([torch.stack([c["t5_cond"] for c in clips]), torch.stack([c["t5_uncond"] for c in clips])])
    idx, dts = vm.euler_tables(a.flow_steps + 1)
    stream = torch.cuda.Stream(device=device)

    ms = {m: [] for m in FORMS}
    last = {}
    with torch.cuda.stream(stream):
        cond = {"lens": eng["lens"].precompute_cond(t5, midi, beats, T, persistent=True, lengths=list(LENGTHS)),
                "equal": eng["equal"].precompute_cond(torch.cat([torch.stack([c["t5_cond"] for c in full]), torch.stack([c["t5_uncond"] for c in full])]),
                                                      torch.stack([c["midi"].reshape(-1) for c in full]), torch.stack([c["beats"].reshape(-1) for c in full]),
                                                      T, persistent=True),
                "single": [eng["single"][b].precompute_cond(torch.stack([c["t5_cond"], c["t5_uncond"]]), c["midi"], c["beats"], LENGTHS[b], persistent=True)
                           for b, c in enumerate(clips)]}
        x_equal = torch.stack([c["x_latent"] for c in full])

        def one_pass(m, k):
            if m == "lens":
                return eng[m].sample_cfg(x, cond[m], idx, dts, a.scale, seed=SEED + k, lengths=list(LENGTHS))
            if m == "equal":
                return eng[m].sample_cfg(x_equal, cond[m], idx, dts, a.scale, seed=SEED + k)
            return [eng[m][b].sample_cfg(clips[b]["x_latent"][None], cond[m][b], idx, dts, a.scale, seed=SEED + k, clip_base=b) for b in range(B)]

        for m in FORMS:
            for k in range(a.warmup):
                z = one_pass(m, k)
            stream.synchronize()
            assert all(bool(torch.isfinite(t).all()) for t in (z if isinstance(z, list) else [z])), m
        for r in range(a.rounds):
            for m in FORMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                last[m] = one_pass(m, a.warmup + r)
                e1.record(stream)
                e1.synchronize()
                ms[m].append(e0.elapsed_time(e1))
            print("round %d: " % r + "  ".join(f"{m} {ms[m][-1]:.2f} ms" for m in FORMS), flush=True)
    med = {m: statistics.median(ms[m]) for m in FORMS}
    mel_s = sum(LENGTHS) * 2 / 75.0
    res = {"workload": f"8 clips of {list(LENGTHS)} latent tokens ({mel_s:.1f} s of mel), {a.flow_steps} Euler steps, bf16 DiT, sampler calls only (graph replay)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_form": a.warmup,
           "graphs": {"lens": eng["lens"].graphs(), "equal": eng["equal"].graphs(), "single": [e.graphs() for e in eng["single"]]},
           "median_ms_per_pass": med, "min_ms_per_pass": {m: min(ms[m]) for m in FORMS}, "max_ms_per_pass": {m: max(ms[m]) for m in FORMS},
           "ms_per_pass": ms,
           "mel_seconds_per_second": {m: mel_s / (med[m] * 1e-3) for m in ("lens", "single")},
           "lens_over_single": med["lens"] / med["single"], "lens_over_equal": med["lens"] / med["equal"],
           "padding_share": 1.0 - sum(LENGTHS) / (B * T),
           "rows_equal_their_single_calls_bit_for_bit": all(bool(torch.equal(last["lens"][b, :, :n], last["single"][b][0])) for b, n in enumerate(LENGTHS))}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
