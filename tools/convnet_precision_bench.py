"""VAE decode + HiFi-GAN per pass in the conv nets' precisions (run on the GPU box): 8 x 20 s clips (BASELINE configs[1]: latent 752 frames ->
mel 1504 -> 481280 samples), one process, HIP-event timing, the modes alternated round by round so that clock drift hits all alike.
    python tools/convnet_precision_bench.py [clips] [rounds]      -> one JSON line (ms per pass: median over the rounds; ratios)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from versband_amd import synth  # noqa: E402
from versband_amd.engine import Context, build_hifigan, build_vae_decoder  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
MODES = ("bf16", "bf16xt", "split", "fp32mf")
T_LAT = 752
ctx = Context("cuda:0")
vcfg, hcfg = synth.VAEConfig(), synth.HifiGanConfig()
sd_v = synth.make_state_dict(synth.vae_decoder_shapes(vcfg), 1235)
sd_h = synth.make_state_dict(synth.hifigan_shapes(hcfg), 1236)
nets = {m: (build_vae_decoder(ctx, sd_v, precision=m), build_hifigan(ctx, sd_h, hcfg.as_hparams(), precision=m)) for m in MODES}
z = torch.from_numpy(synth.prng.normal(77, B * 20 * T_LAT).reshape(B, 20, T_LAT)).float().cuda()


def one_pass(m):
    vae, voc = nets[m]
    return voc.run(vae.run(z))


def timed(m):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    vae, voc = nets[m]
    e[0].record()
    mel = vae.run(z)
    e[1].record()
    voc.run(mel)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


for m in MODES:            # warm-up: workspaces, first-launch attributes, clocks
    for _ in range(2):
        one_pass(m)
torch.cuda.synchronize()
ms = {m: [] for m in MODES}
for r in range(ROUNDS):
    for m in (MODES if r % 2 == 0 else MODES[::-1]):
        ms[m].append(timed(m))
res = {"clips": B, "rounds": ROUNDS}
for m in MODES:
    res[m] = {"vae_ms": round(statistics.median(v for v, _ in ms[m]), 3), "vocoder_ms": round(statistics.median(h for _, h in ms[m]), 3),
              "vae_ms_min_max": [round(min(v for v, _ in ms[m]), 3), round(max(v for v, _ in ms[m]), 3)],
              "vocoder_ms_min_max": [round(min(h for _, h in ms[m]), 3), round(max(h for _, h in ms[m]), 3)],
              "pass_ms": round(statistics.median(v + h for v, h in ms[m]), 3),
              "pass_ms_min_max": [round(min(v + h for v, h in ms[m]), 3), round(max(v + h for v, h in ms[m]), 3)]}
res["bf16_over_split"] = round(res["bf16"]["pass_ms"] / res["split"]["pass_ms"], 4)
res["bf16xt_vae_over_bf16_vae"] = round(res["bf16xt"]["vae_ms"] / res["bf16"]["vae_ms"], 4)
res["bf16xt_vae_over_split_vae"] = round(res["bf16xt"]["vae_ms"] / res["split"]["vae_ms"], 4)
res["bf16_over_fp32mf"] = round(res["bf16"]["pass_ms"] / res["fp32mf"]["pass_ms"], 4)
print(json.dumps(res))
