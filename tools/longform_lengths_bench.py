"""Long clips of different lengths through sample_long(mode="joint"): ONE call with window rows (lengths=) against one call per clip.

One process, one GPU: 4 clips of 1800, 2200, 2600 and 3000 latent tokens, windows of 1500 tokens, overlap 128 - 9 full-length rows in
groups of 2 / 2 / 2 / 3 (longform.plan_window_rows) - 50 Euler steps x 2 NFE, bf16 DiT, synthetic weights.  The sampler alone is timed
(cutting the rows, conditioning, step loop, stitch), with HIP events on the pass's stream, three warm-up passes first (a key's second call captures its
step loop's graph; the graphs each engine holds at the end are reported), then the two forms alternated over --rounds rounds.
Reported: the median ms per pass of each form and their ratio.  The gate: the one call takes less time than the four calls together, by
median of at least 5 rounds of the same run; the exit status is 1 when it does not.

    python tools/longform_lengths_bench.py [--rounds 7] [--out profiles/longform_lengths_bench.json]
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

FORMS = ("per_clip", "window_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="+", default=[1800, 2200, 2600, 3000])
    ap.add_argument("--flow-steps", type=int, default=50)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.warmup >= 0, "the gate is a median of at least 5 rounds"
    if not torch.cuda.is_available():
        raise SystemExit("longform_lengths_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED
    from versband_amd import longform
    from versband_amd import model as vm
    from versband_amd import synth
    from versband_amd.engine import Context, DiTEngine

    device = torch.device("cuda:0")
    dcfg = synth.DiTConfig()
    ctx = Context(device)
    sd = synth.make_state_dict(synth.dit_shapes(dcfg), SEED)
    base = DiTEngine(ctx, dcfg, sd, precision="bf16")
    # one engine handle per form (shared packed weights): each keeps its own buffers and graph cache
    engines = {"per_clip": base, "window_rows": DiTEngine(ctx, dcfg, sd, precision="bf16", share=base)}
    lengths, B, Tmax = a.lengths, len(a.lengths), max(a.lengths)
    clips = [{k: v.to(device) for k, v in synth.make_clip_inputs(SEED, b, n, L=80).items()} for b, n in enumerate(lengths)]
    x0 = torch.zeros(B, dcfg.in_channels, Tmax, device=device)
    midi, beats = torch.zeros(B, 1, 2 * Tmax, dtype=torch.int64, device=device), torch.zeros(B, 1, 2 * Tmax, dtype=torch.int64, device=device)
    for b, (c, n) in enumerate(zip(clips, lengths)):
        x0[b, :, :n], midi[b, :, :2 * n], beats[b, :, :2 * n] = c["x_latent"], c["midi"], c["beats"]
    tc, tu = torch.stack([c["t5_cond"] for c in clips]), torch.stack([c["t5_uncond"] for c in clips])
    idx, dts = vm.euler_tables(a.flow_steps + 1)
    group, start, row_len = longform.plan_window_rows(lengths, dcfg.max_len, a.overlap)
    stream = torch.cuda.Stream(device=device)
    kw = dict(window=dcfg.max_len, overlap=a.overlap, mode="joint")

    def one_pass(form, k):
        if form == "window_rows":
            return longform.sample_long(engines[form], x0, tc, tu, midi, beats, idx, dts, a.scale, seed=SEED + k, lengths=lengths, **kw)
        z = torch.zeros_like(x0)
        for b, (c, n) in enumerate(zip(clips, lengths)):
            z[b:b + 1, :, :n] = longform.sample_long(engines[form], c["x_latent"][None], tc[b:b + 1], tu[b:b + 1], c["midi"][None], c["beats"][None],
                                                     idx, dts, a.scale, seed=SEED + k, clip_base=b, **kw)
        return z

    ms = {f: [] for f in FORMS}
    with torch.cuda.stream(stream):
        z = {}
        for f in FORMS:
            for k in range(a.warmup):
                z[f] = one_pass(f, k)
            stream.synchronize()
            assert tuple(z[f].shape) == (B, dcfg.in_channels, Tmax) and bool(torch.isfinite(z[f]).all()), f
        same = bool(torch.equal(z["per_clip"], z["window_rows"])) if a.warmup else None      # the contract: the same bits
        for r in range(a.rounds):
            for f in FORMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                one_pass(f, a.warmup + r)
                e1.record(stream)
                e1.synchronize()
                ms[f].append(e0.elapsed_time(e1))
            print("round %d: " % r + "  ".join(f"{f} {ms[f][-1]:.2f} ms" for f in FORMS), flush=True)
    med = {f: statistics.median(ms[f]) for f in FORMS}
    res = {"workload": f"{B} clips of {lengths} latent tokens, windows of {dcfg.max_len} overlapping by {a.overlap}: {len(group)} rows of {sorted(set(row_len))} "
                       f"tokens in groups of {[group.count(b) for b in range(B)]}, {a.flow_steps} Euler steps x 2 NFE, bf16 DiT, sampler only "
                       "(rows + conditioning + step loop + stitch)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_form": a.warmup,
           "graphs": {f: engines[f].graphs() for f in FORMS}, "same_bits": same,
           "median_ms_per_pass": med, "ms_per_pass": ms, "window_rows_over_per_clip": med["window_rows"] / med["per_clip"],
           "gate": "median(window_rows) < median(per_clip)", "gate_ok": med["window_rows"] < med["per_clip"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0 if res["gate_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
