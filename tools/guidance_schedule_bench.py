"""What a guidance schedule costs: the sampler's step loop under four forms of one call, side by side.

    plain     the constant-scale call (the yardstick: same build, same run)
    interval  guidance_interval_weights(lo = 0.25, hi = 0.75): the middle half of the steps guided, the others single-branch
    zeros     every step single-branch, in the two-branch layout
    one       an n_branch = 1 call on conditioning precomputed for the conditional branch alone

One process, one GPU: 8 clips x 20 s, 50 Euler steps, bf16 DiT, synthetic weights.  The sampler call alone is timed (the conditioning is
precomputed once per form, outside the timing), graph replay, with HIP events on the pass's stream, two warm-up passes per form (the second
captures the step loop's graph), then the forms alternated over --rounds rounds.  Reported: median and min .. max ms per pass of each form
and the ratios to the plain call.  There is no gate.  The forms are also checked against each other: zeros equals one bit for bit (at this
size the router counts its buckets, the path the small test shapes do not reach), interval differs from plain and equals itself with
the bucket counts as a launch of their own (VB_BUCKET_COUNT_LAUNCH).

    python tools/guidance_schedule_bench.py [--rounds 7] [--out profiles/guidance_schedule.json]
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

FORMS = ("plain", "interval", "zeros", "one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--flow-steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--lo", type=float, default=0.25)
    ap.add_argument("--hi", type=float, default=0.75)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 2, "the second warm-up pass captures the graph"
    if not torch.cuda.is_available():
        raise SystemExit("guidance_schedule_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED, clip_batch
    from versband_amd import model as vm
    from versband_amd import synth
    from versband_amd.engine import Context, DiTEngine

    device = torch.device("cuda:0")
    T_mel = (int(round(a.seconds * 75.0)) + 7) // 8 * 8
    T = T_mel // 2
    dcfg = synth.DiTConfig()
    ctx = Context(device)
    sd = synth.make_state_dict(synth.dit_shapes(dcfg), SEED)
    base = DiTEngine(ctx, dcfg, sd, precision="bf16")
    # one engine handle per form (shared packed weights): each keeps its own buffers and graph cache
    engines = {m: (base if i == 0 else DiTEngine(ctx, dcfg, sd, precision="bf16", share=base)) for i, m in enumerate(FORMS)}
    inp = {k: v.to(device) for k, v in clip_batch(a.batch, T, 80, seed=SEED).items()}
    idx, dts = vm.euler_tables(a.flow_steps + 1)
    weights = {"plain": None, "interval": vm.guidance_interval_weights(a.flow_steps + 1, a.lo, a.hi), "zeros": [0.0] * a.flow_steps, "one": None}
    guided_steps = int(sum(weights["interval"]))
    stream = torch.cuda.Stream(device=device)

    ms = {m: [] for m in FORMS}
    last = {}
    with torch.cuda.stream(stream):
        t5_two = torch.cat([inp["t5_cond"], inp["t5_uncond"]])
        cond = {m: engines[m].precompute_cond(inp["t5_cond"] if m == "one" else t5_two, inp["midi"], inp["beats"], T, persistent=True) for m in FORMS}

        def one_pass(m, k):
            return engines[m].sample_cfg(inp["x_latent"], cond[m], idx, dts, 1.0 if m == "one" else a.scale, seed=SEED + k, guidance=weights[m])

        for m in FORMS:
            for k in range(a.warmup):
                z = one_pass(m, k)
            stream.synchronize()
            assert tuple(z.shape) == (a.batch, dcfg.in_channels, T) and bool(torch.isfinite(z).all()), m
        for r in range(a.rounds):
            for m in FORMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                last[m] = one_pass(m, a.warmup + r)
                e1.record(stream)
                e1.synchronize()
                ms[m].append(e0.elapsed_time(e1))
            print("round %d: " % r + "  ".join(f"{m} {ms[m][-1]:.2f} ms" for m in FORMS), flush=True)
        # the interval form once more with the bucket counts as a launch of their own (VB_BUCKET_COUNT_LAUNCH: bit-identical by
        # construction): the router's count tables survive the changes between one and two branches
        os.environ["VB_BUCKET_COUNT_LAUNCH"] = "1"
        ctx.lib.vb_tune_reload()
        check = engines["interval"].sample_cfg(inp["x_latent"], cond["interval"], idx, dts, a.scale, seed=SEED + a.warmup + a.rounds - 1, guidance=weights["interval"])
        stream.synchronize()
        del os.environ["VB_BUCKET_COUNT_LAUNCH"]
        ctx.lib.vb_tune_reload()
    med = {m: statistics.median(ms[m]) for m in FORMS}
    res = {"workload": f"{a.batch} x {T_mel / 75.0:.1f} s, T_lat={T}, {a.flow_steps} Euler steps, bf16 DiT, sampler call only (graph replay)",
           "interval": [a.lo, a.hi], "guided_steps_of_interval": guided_steps,
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_form": a.warmup,
           "graphs": {m: engines[m].graphs() for m in FORMS},
           "median_ms_per_pass": med, "min_ms_per_pass": {m: min(ms[m]) for m in FORMS}, "max_ms_per_pass": {m: max(ms[m]) for m in FORMS},
           "ms_per_pass": ms,
           "interval_over_plain": med["interval"] / med["plain"], "zeros_over_plain": med["zeros"] / med["plain"], "zeros_over_one": med["zeros"] / med["one"],
           "zeros_equals_one_bit_for_bit": bool(torch.equal(last["zeros"], last["one"])),
           "interval_equals_its_count_launch_form": bool(torch.equal(last["interval"], check)),
           "interval_differs_from_plain": not bool(torch.equal(last["interval"], last["plain"]))}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
