"""The three modes of longform.sample_long side by side: crossfade (independent windows, one batched call), continue (windows in order,
each held to the previous one: nw calls of B rows) and joint (one batched call, overlaps reconciled after every step).

One process, one GPU, the long-form workload of `bench.py --workload c5`: 4 clips x 120 s (T = 4500 latent frames, windows of 1500 tokens,
overlap 128), 50 Euler steps x 2 NFE, bf16 DiT, synthetic weights.  The sampler alone is timed (conditioning + step loop + stitch; the VAE
and the vocoder are the same work in every mode), with HIP events on the pass's stream, two warm-up passes per mode (the second captures
the step loop's graph), then the modes alternated over --rounds rounds.  Reported: the median ms per pass of each mode and the two ratios
joint / crossfade and continue / joint.  There is no gate: the yardsticks are the two existing modes in the same build and run.

    python tools/longform_modes_bench.py [--rounds 5] [--out profiles/longform_modes.json]
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

MODES = ("crossfade", "continue", "joint")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--flow-steps", type=int, default=50)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="write the result (raw per-pass times included) as JSON")
    a = ap.parse_args()
    assert a.rounds >= 1 and a.warmup >= 0
    if not torch.cuda.is_available():
        raise SystemExit("longform_modes_bench: no GPU - this is a measurement, there is nothing to report without one")

    from tests.helpers import SEED, clip_batch
    from versband_amd import longform
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
    # one engine handle per mode (shared packed weights): each keeps its own buffers and graph cache, as three services would
    engines = {m: (base if i == 0 else DiTEngine(ctx, dcfg, sd, precision="bf16", share=base)) for i, m in enumerate(MODES)}
    inp = {k: v.to(device) for k, v in clip_batch(a.batch, T, 80, seed=SEED).items()}
    idx, dts = vm.euler_tables(a.flow_steps + 1)
    times = vm.euler_times(a.flow_steps + 1)
    plan = longform.plan_windows(T, dcfg.max_len, a.overlap)
    stream = torch.cuda.Stream(device=device)

    def one_pass(mode, k):
        kw = dict(t_next=times, sigma_min=1e-4) if mode == "continue" else {}
        return longform.sample_long(engines[mode], inp["x_latent"], inp["t5_cond"], inp["t5_uncond"], inp["midi"], inp["beats"], idx, dts,
                                    a.scale, window=dcfg.max_len, overlap=a.overlap, seed=SEED + k, mode=mode, **kw)

    ms = {m: [] for m in MODES}
    with torch.cuda.stream(stream):
        for m in MODES:
            for k in range(a.warmup):
                z = one_pass(m, k)
            stream.synchronize()
            assert tuple(z.shape) == (a.batch, dcfg.in_channels, T) and bool(torch.isfinite(z).all()), m
        for r in range(a.rounds):
            for m in MODES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                one_pass(m, a.warmup + r)
                e1.record(stream)
                e1.synchronize()
                ms[m].append(e0.elapsed_time(e1))
            print("round %d: " % r + "  ".join(f"{m} {ms[m][-1]:.2f} ms" for m in MODES), flush=True)
    med = {m: statistics.median(ms[m]) for m in MODES}
    res = {"workload": f"{a.batch} x {T_mel / 75.0:.1f} s, T_lat={T}, windows at {[s for s, _ in plan]} of {plan[0][1]} tokens, "
                       f"{a.flow_steps} Euler steps x 2 NFE, bf16 DiT, sampler only (conditioning + step loop + stitch)",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "warmup_passes_per_mode": a.warmup,
           "graphs": {m: engines[m].graphs() for m in MODES},
           "median_ms_per_pass": med, "ms_per_pass": ms,
           "joint_over_crossfade": med["joint"] / med["crossfade"], "continue_over_joint": med["continue"] / med["joint"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
