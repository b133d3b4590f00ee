"""Path-level parity on the GPU: DiT forward / CFG sampler / VAE decode / HiFi-GAN against the
golden fixtures produced by the REAL reference (tests/golden, oracle/gen_golden.py) and against the
CPU oracle at other sizes, through the reference-shaped host API (versband_amd.model) and the C ABI.

Tolerances (north_star): mel-latent relative error <= 1e-3 and mel L1 < 1e-3 in parity ("split")
mode with bit-exact routing indices on identical injected noise; the bf16 production mode is
measured against the same oracle and its routing flip rate is reported, not asserted to be zero."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, check_digest, clip_batch, describe, exp_noise, gumbel_arrays, gumbel_arrays_steps, rel_l2
from versband_amd import _lib as L
from versband_amd import model as vm
from versband_amd import prng
from versband_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Context("cuda:0")


@pytest.fixture(scope="module")
def sds():
    return {E: synth.make_state_dict(synth.dit_shapes(synth.DiTConfig(num_experts=E)), SEED) for E in (4, 8)}


@pytest.fixture(scope="module")
def engines(ctx, sds):
    from versband_amd.engine import DiTEngine
    out = {}
    for E in (4, 8):
        for prec in ("split", "bf16"):
            if E == 8 and prec == "bf16":
                continue
            out[(E, prec)] = DiTEngine(ctx, synth.DiTConfig(num_experts=E), sds[E], precision=prec)
    return out


def _golden_forward_inputs(tag):
    g = np.load(os.path.join(GOLD, f"dit_forward_{tag}.npz"))
    B, T, Lc, E, _ = [int(v) for v in g["meta"]]
    noise = [[tuple(torch.from_numpy(g[f"noise{br}_{i}_{j}"]) for j in range(3)) for i in range(4)] for br in (0, 1)]
    return g, B, T, Lc, E, noise


@pytest.mark.parametrize("tag,E", [("e4", 4), ("e8", 8)])
def test_dit_forward_vs_reference_golden_split(engines, sds, tag, E):
    g, B, T, Lc, E_, noise = _golden_forward_inputs(tag)
    eng = engines[(E, "split")]
    t5 = torch.cat([torch.from_numpy(g["t5_cond"]), torch.from_numpy(g["t5_uncond"])])
    cond = eng.precompute_cond(t5, torch.from_numpy(g["midi"]), torch.from_numpy(g["beats"]), T)
    t_idx = torch.from_numpy(np.concatenate([g["t_idx"], g["t_idx"]]))
    v, routes = eng.forward(torch.from_numpy(g["x"]), t_idx, cond, noise=gumbel_arrays(noise), return_routes=True)
    torch.cuda.synchronize()
    ref = np.concatenate([g["v0"], g["v1"]])
    assert rel_l2(v, ref) < 1e-4, describe("dit_forward(split) vs reference", v, ref)
    # routing indices: bit-exact vs the oracle's on identical noise
    sd = sds[E]
    x = torch.from_numpy(g["x"])
    for br, key in ((0, "t5_cond"), (1, "t5_uncond")):
        c = ref_cpu.dit_precompute(sd, torch.from_numpy(g[key]), torch.from_numpy(g["midi"]), torch.from_numpy(g["beats"]), T)
        _, aux = ref_cpu.dit_forward(sd, x, torch.from_numpy(g["t_idx"]), c, noise[br], return_aux=True)
        N = B * T
        for i in range(4):
            got_c = routes[i, 0, br * N:(br + 1) * N].cpu().long()
            got_a = routes[i, 1, br * N:(br + 1) * N].cpu().long()
            assert torch.equal(got_c, aux[f"ic{i}"]), f"block {i} caption routing differs ({int((got_c != aux[f'ic{i}']).sum())} tokens)"
            assert torch.equal(got_a, aux[f"ia{i}"]), f"block {i} acoustic routing differs"


def test_sample_cfg_and_decode_vs_reference_golden(ctx, engines, sds):
    from versband_amd.engine import build_vae_decoder
    g = np.load(os.path.join(GOLD, "sample_cfg_3step.npz"))
    B, T, Lc, E, seed, steps = [int(v) for v in g["meta"]]
    eng = engines[(E, "split")]
    t5 = torch.cat([torch.from_numpy(g["t5_cond"]), torch.from_numpy(g["t5_uncond"])])
    cond = eng.precompute_cond(t5, torch.from_numpy(g["midi"]), torch.from_numpy(g["beats"]), T)
    noise_steps = [[exp_noise(B, T, E, 2 * k + br, 4) for br in (0, 1)] for k in range(steps)]
    idx, dts = vm.euler_tables(steps + 1)
    x, traj = eng.sample_cfg(torch.from_numpy(g["x"]), cond, idx, dts, float(g["scale"]), noise=gumbel_arrays_steps(noise_steps),
                             return_traj=True)
    torch.cuda.synchronize()
    assert rel_l2(traj, g["traj"]) < 1e-3, describe("trajectory vs reference", traj, g["traj"])
    assert rel_l2(x, g["z"]) < 1e-3, describe("latent vs reference", x, g["z"])
    sdv = synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1)
    vae = build_vae_decoder(ctx, sdv, scale_factor=float(g["scale_factor"]))
    mel = vae.run(x)
    torch.cuda.synchronize()
    l1 = float((mel.cpu() - torch.from_numpy(g["mel"])).abs().mean())
    assert l1 < 1e-3, f"mel L1 {l1:.3e}; " + describe("mel vs reference", mel, g["mel"])


def _f64(sd):
    """a state dict in float64: the oracle follows the dtype of its inputs"""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("fp32mf", 2e-5), ("split", 2e-4)])
def test_vae_decode_vs_golden_and_oracle(ctx, prec, tol):
    """T = 151: the latent-rate layers fall back from minimal filtering to the direct kernels in fp32mf (length not a multiple of 4);
    T = 148: every eligible layer runs minimal filtering, the length still not a tile multiple.  Oracle in float64."""
    from versband_amd.engine import build_vae_decoder
    sdv = synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1)
    vae = build_vae_decoder(ctx, sdv, precision=prec)
    g = np.load(os.path.join(GOLD, "vae_decode.npz"))
    mel = vae.run(torch.from_numpy(g["z"]))
    torch.cuda.synchronize()
    assert rel_l2(mel, g["mel"]) < tol, describe("vae_decode vs reference", mel, g["mel"])
    if prec == "fp32mf":                                  # (the mode really took the minimal-filtering kernels)
        mel32 = build_vae_decoder(ctx, sdv, precision="fp32").run(torch.from_numpy(g["z"]))
        torch.cuda.synchronize()
        assert not torch.equal(mel, mel32)
    # ragged lengths (not a tile multiple) vs the oracle
    for T in (151, 148):
        z = torch.from_numpy(synth.prng.normal(77, 1 * 20 * T).reshape(1, 20, T))
        ref = ref_cpu.vae_decode(_f64(sdv), z.double())
        mel = vae.run(z)
        torch.cuda.synchronize()
        assert mel.shape == ref.shape
        assert rel_l2(mel, ref) < tol, describe(f"vae_decode T={T} vs oracle", mel, ref)


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("fp32mf", 2e-5), ("split", 2e-4)])
def test_vae_encode_vs_golden_and_oracle(ctx, prec, tol):
    """Encoder1D (k5 ResnetBlocks, stride-2 Downsample1D as two polyphase convolutions, mid attention) +
    quant_conv through vb_vae_encode; posterior sample/mode through the reference-named API.  T_mel = 302 (151 latent frames: those
    layers fall back to the direct kernels in fp32mf) and 296 (every eligible layer runs minimal filtering); oracle in float64."""
    from versband_amd.engine import build_vae_encoder
    from versband_amd.model import DiagonalGaussianDistribution
    sde = synth.make_state_dict(synth.vae_encoder_shapes(synth.VAEConfig()), SEED + 3)
    enc = build_vae_encoder(ctx, sde, precision=prec)
    g = np.load(os.path.join(GOLD, "vae_encode.npz"))
    mom = enc.run(torch.from_numpy(g["x"]))
    torch.cuda.synchronize()
    assert rel_l2(mom, g["moments"]) < tol, describe("vae_encode vs reference", mom, g["moments"])
    post = DiagonalGaussianDistribution(mom)
    assert rel_l2(post.sample(torch.from_numpy(g["eps"])), g["z"]) < tol
    assert rel_l2(post.mode(), g["mode"]) < tol
    if prec == "fp32mf":                                  # (the mode really took the minimal-filtering kernels)
        mom32 = build_vae_encoder(ctx, sde, precision="fp32").run(torch.from_numpy(g["x"]))
        torch.cuda.synchronize()
        assert not torch.equal(mom, mom32)
    # ragged mel lengths (not a tile multiple) vs the oracle
    for T_mel in (302, 296):
        x = torch.from_numpy(synth.prng.normal(78, 1 * 80 * T_mel).reshape(1, 80, T_mel))
        ref = ref_cpu.vae_encode(_f64(sde), x.double())
        mom = enc.run(x)
        torch.cuda.synchronize()
        assert mom.shape == ref.shape
        assert rel_l2(mom, ref) < tol, describe(f"vae_encode T_mel={T_mel} vs oracle", mom, ref)
    with pytest.raises(ValueError):
        enc.run(torch.zeros(1, 80, 301))          # odd mel length cannot be halved (the reference pads to a multiple of 8 upstream)


@pytest.mark.parametrize("tag", ["v1", "rb2"])
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("fp32mf", 2e-5), ("split", 2e-4)])
def test_hifigan_vs_golden_and_oracle(ctx, tag, prec, tol):
    """B = 2, T = 37: conv_pre falls back to the direct kernel in fp32mf; B = 3, T = 36: every eligible layer runs minimal filtering.
    Oracle in float64."""
    from versband_amd.engine import build_hifigan
    cfg = synth.HifiGanConfig() if tag == "v1" else synth.HifiGanConfig(
        resblock="2", upsample_rates=(8, 8, 5), upsample_kernel_sizes=(16, 16, 11), upsample_initial_channel=128,
        resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 3), (1, 3)))
    sd = synth.make_state_dict(synth.hifigan_shapes(cfg), SEED + 2)
    net = build_hifigan(ctx, sd, cfg.as_hparams(), precision=prec)
    g = np.load(os.path.join(GOLD, f"hifigan_{tag}.npz"))
    wav = net.run(torch.from_numpy(g["mel"]))
    torch.cuda.synchronize()
    assert wav.shape == g["wav"].shape
    assert rel_l2(wav, g["wav"]) < tol, describe("hifigan vs reference", wav, g["wav"])
    if prec == "fp32mf":                                  # (the mode really took the minimal-filtering kernels)
        wav32 = build_hifigan(ctx, sd, cfg.as_hparams(), precision="fp32").run(torch.from_numpy(g["mel"]))
        torch.cuda.synchronize()
        assert not torch.equal(wav, wav32)
    for B, T in ((2, 37), (3, 36)):
        mel = torch.from_numpy(synth.prng.uniform(5, B * 80 * T, -5.0, 1.5).reshape(B, 80, T))
        ref = ref_cpu.hifigan_forward(_f64(sd), cfg.as_hparams(), mel.double())
        wav = net.run(mel)
        torch.cuda.synchronize()
        assert wav.shape == ref.shape
        assert rel_l2(wav, ref) < tol, describe(f"hifigan B={B} T={T} vs oracle", wav, ref)


def test_reference_api_end_to_end_vs_oracle(tmp_path):
    """configs/vocal2music.yaml -> instantiate_from_config -> load_state_dict -> CFMSampler.sample_cfg ->
    decode_first_stage -> HifiGAN, exactly the call sequence of scripts/test_final.py:140-151,388-421."""
    import yaml
    from ldm.models.diffusion.cfm1_audio_sampler import CFMSampler
    from ldm.util import instantiate_from_config
    from vocoder.hifigan import HifiGAN
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    config = vm.load_config(os.path.join(root, "configs", "vocal2music.yaml"))
    config.model.params["precision"] = "split"
    model = instantiate_from_config(config.model)
    dcfg, vcfg, hcfg = synth.DiTConfig(), synth.VAEConfig(), synth.HifiGanConfig()
    sd_d = synth.make_state_dict(synth.dit_shapes(dcfg), SEED)
    sd_v = synth.make_state_dict(synth.vae_decoder_shapes(vcfg), SEED + 1)
    sd_h = synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2)
    ckpt = {"state_dict": {**{"model.diffusion_model." + k: v for k, v in sd_d.items()},
                           **{"first_stage_model." + k: v for k, v in sd_v.items()}, "scale_factor": torch.tensor(0.9)}}
    torch.save(ckpt, tmp_path / "last.ckpt")
    model.load_state_dict(torch.load(tmp_path / "last.ckpt", map_location="cpu")["state_dict"], strict=False)
    model = model.to("cuda:0")
    sampler = CFMSampler(model, num_timesteps=1000)
    vdir = tmp_path / "hifigan"
    vdir.mkdir()
    yaml.safe_dump(hcfg.as_hparams(), open(vdir / "config.yaml", "w"))
    torch.save({"state_dict": {"model_gen": sd_h}}, vdir / "model_ckpt_steps_100.ckpt")
    torch.save({"state_dict": {"model_gen": {}}}, vdir / "model_ckpt_steps_7.ckpt")     # older ckpt must be ignored
    vocoder = HifiGAN(vocoder_ckpt=str(vdir), device="cuda:0")

    B, T, Lc, E, steps, scale = 2, 20, 8, 4, 2, 3.0
    inp = clip_batch(B, T, Lc)
    ac = {"acoustic": torch.zeros(B, 20, 2 * T), "midi": inp["midi"], "beats": inp["beats"]}
    c = model.get_learned_conditioning({"caption": inp["t5_cond"], "acoustic": ac, "name": ["a"] * B})
    uc = model.get_learned_conditioning({"caption": inp["t5_uncond"], "acoustic": ac, "name": ["a"] * B})
    noise_steps = [[exp_noise(B, T, E, 2 * k + br, 4) for br in (0, 1)] for k in range(steps)]
    shape = [sampler.model.first_stage_model.embed_dim, T]
    z, _ = sampler.sample_cfg(S=100, cond=c, batch_size=B, shape=shape, verbose=False, unconditional_guidance_scale=scale,
                              unconditional_conditioning=uc, x_T=inp["x_latent"], x_latent=inp["x_latent"], timesteps=steps + 1,
                              gumbel_noise=gumbel_arrays_steps(noise_steps))
    mel = sampler.model.decode_first_stage(z)
    wav = vocoder(mel[0].transpose(0, 1).cpu())
    # oracle
    cc = ref_cpu.dit_precompute(sd_d, inp["t5_cond"], inp["midi"], inp["beats"], T)
    cu = ref_cpu.dit_precompute(sd_d, inp["t5_uncond"], inp["midi"], inp["beats"], T)
    z_ref = ref_cpu.sample_cfg(sd_d, inp["x_latent"], cc, cu, scale, steps + 1, lambda k, br: noise_steps[k][br])
    mel_ref = ref_cpu.vae_decode(sd_v, z_ref, scale_factor=0.9)
    wav_ref = ref_cpu.hifigan_forward(sd_h, hcfg.as_hparams(), mel_ref[:1]).view(-1)
    assert rel_l2(z, z_ref) < 1e-3, describe("z", z, z_ref)
    assert float((mel.cpu() - mel_ref).abs().mean()) < 1e-3, describe("mel", mel, mel_ref)
    assert wav.shape == (2 * T * hcfg.hop,) and wav.dtype == np.float32
    assert rel_l2(wav, wav_ref) < 1e-3, describe("wav", wav, wav_ref)


def test_determinism_and_clip_keyed_noise(engines):
    """same inputs twice -> identical bits (doubles as a race detector for the LDS kernels); device-drawn
    router noise is keyed by the global clip index, so a clip's result does not depend on its batch slot."""
    eng = engines[(4, "bf16")]
    B, T, Lc = 3, 40, 8
    inp = clip_batch(B, T, Lc)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]])
    cond = eng.precompute_cond(t5, inp["midi"], inp["beats"], T)
    idx, dts = vm.euler_tables(4)
    a = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=5, clip_base=0)
    b = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=5, clip_base=0)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # clip 2 alone (clip_base=2) == clip 2 inside the batch
    sel = slice(2, 3)
    t5s = torch.cat([inp["t5_cond"][sel], inp["t5_uncond"][sel]])
    cond1 = eng.precompute_cond(t5s, inp["midi"][sel], inp["beats"][sel], T)
    c = eng.sample_cfg(inp["x_latent"][sel], cond1, idx, dts, 3.0, seed=5, clip_base=2)
    torch.cuda.synchronize()
    assert torch.equal(a[sel], c), describe("clip 2 alone vs in batch", c, a[sel])


def test_sampler_graph_replay_equals_eager(ctx, sds, monkeypatch):
    """vb_sample_cfg captures its step loop into a hipGraph the second time a call arrives with the same buffers on a capturable
    stream and replays it afterwards; the noise key (seed / clip base) travels through device memory, so replays with OTHER seeds
    must equal eager runs of those seeds bit for bit.  A stale persistent conditioning handle is refused."""
    from versband_amd._lib import VersbandError
    from versband_amd.engine import DiTEngine
    eng = DiTEngine(ctx, synth.DiTConfig(), sds[4], precision="bf16")
    B, T, Lc = 2, 120, 16
    inp = clip_batch(B, T, Lc)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).cuda()
    midi, beats = inp["midi"].cuda(), inp["beats"].cuda()
    idx, dts = vm.euler_tables(6)
    stream = torch.cuda.Stream()
    outs = {}
    with torch.cuda.stream(stream):
        for rep, seed in enumerate((5, 5, 9, 13)):
            cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
            outs[(seed, rep)] = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=seed, clip_base=rep)
        stream.synchronize()
        assert eng.graphs() == 1, "the repeated call was not captured"
        # another engine of another shape runs, is destroyed and its memory returned to the driver between capture and replay (this
        # sequence exposed a hipMemsetAsync node of the captured loop going wrong on ROCm 7.2: the loop now has kernel nodes only)
        other = DiTEngine(ctx, synth.DiTConfig(), sds[4], precision="bf16", share=eng)
        big = clip_batch(5, 200, Lc)
        other.sample_cfg(big["x_latent"], other.precompute_cond(torch.cat([big["t5_cond"], big["t5_uncond"]]), big["midi"], big["beats"], 200),
                         idx, dts, 3.0, seed=1)
        stream.synchronize()
        del other, big
        torch.cuda.empty_cache()
        cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
        again = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=13, clip_base=3)
        stream.synchronize()
        assert torch.equal(again, outs[(13, 3)]) and torch.isfinite(again).all()
        stale = cond
        eng.precompute_cond(t5, midi, beats, T, persistent=True)
        with pytest.raises(VersbandError):
            eng.sample_cfg(inp["x_latent"], stale, idx, dts, 3.0, seed=5)
    monkeypatch.setenv("VB_NO_GRAPH", "1")
    L.load().vb_tune_reload()
    eager = DiTEngine(ctx, synth.DiTConfig(), sds[4], precision="bf16", share=eng)
    with torch.cuda.stream(stream):
        for rep, seed in enumerate((5, 5, 9, 13)):
            cond = eager.precompute_cond(t5, midi, beats, T, persistent=True)
            ref = eager.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=seed, clip_base=rep)
            stream.synchronize()
            assert torch.equal(ref, outs[(seed, rep)]), describe(f"graph replay vs eager, seed {seed} call {rep}", outs[(seed, rep)], ref)
    assert eager.graphs() == 0
    monkeypatch.delenv("VB_NO_GRAPH")
    L.load().vb_tune_reload()
    assert not torch.equal(outs[(5, 1)], outs[(9, 2)])


def test_fused_glue_launches_are_bit_identical(engines, monkeypatch):
    """Round 5: (a) the router adds every token to its bucket's count table (ping-pong tables cleared by the place kernel) instead of a
    count launch per block; (b) FinalLayer, the CFG combination, the Euler update and the step counter's advance are one launch per step
    (a wave holds both branches' velocities of its tokens).  Same integers, same fused multiply-adds: a whole sampler call - an odd number
    of steps so that the ping-pong parity crosses call boundaries - must be bit-identical with either switch back on the separate launches,
    and so must a stand-alone network evaluation with its routes."""
    T, Lc, B = 752, 80, 3           # 4512 token rows: the two-kernel bucket form (N > 4096), ragged last 256-token block
    eng = engines[(4, "bf16")]
    inp = clip_batch(B, T, Lc)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]])
    idx, dts = vm.euler_tables(4)   # 3 steps
    t_idx = torch.full((2 * B,), 640, dtype=torch.int64)
    outs = []
    try:
        for knob in (None, "VB_BUCKET_COUNT_LAUNCH", "VB_EULER_LAUNCH"):
            if knob:
                monkeypatch.setenv(knob, "1")
            L.load().vb_tune_reload()
            cond = eng.precompute_cond(t5, inp["midi"], inp["beats"], T)
            z1 = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=21)
            z2 = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=22)      # a second call: tables as the first one left them
            v, r = eng.forward(inp["x_latent"], t_idx, cond, seed=3, return_routes=True)
            torch.cuda.synchronize()
            outs.append((z1.clone(), z2.clone(), v.clone(), r.clone()))
            if knob:
                monkeypatch.delenv(knob)
    finally:                          # a failure mid-loop must not leave the knob in the library's cached tuning for the next tests
        for knob in ("VB_BUCKET_COUNT_LAUNCH", "VB_EULER_LAUNCH"):
            monkeypatch.delenv(knob, raising=False)
        L.load().vb_tune_reload()
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], outs[0][1])
    for k in (1, 2):
        for j, what in enumerate(("sample seed 21", "sample seed 22", "velocity", "routes")):
            assert torch.equal(outs[0][j], outs[k][j]), describe(f"fused glue vs separate launches (switch {k}, {what})", outs[k][j], outs[0][j])


def test_gemm_tile_configurations_round_alike(engines, monkeypatch):
    """The launcher picks the GEMM tile shape (128x128 two-per-CU kernel, the 192x192 one-per-CU kernel, or 64x64 / 128x64 tiles
    for one or two clips) from the problem size, i.e. from the batch: both must produce bit-identical DiT outputs and routes, otherwise a clip's
    result would depend on the batch it rides in (hard routing amplifies a 1-ulp difference into an expert flip)."""
    eng = engines[(4, "bf16")]
    B, T, Lc = 2, 752, 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 321, dtype=torch.int64)
    outs = []
    for cfg in ("22", "33", "11", "21", "23"):       # 23 = 128 x 192 two-per-CU gated-residual kernel (other launches keep 128 x 128)
        monkeypatch.setenv("VB_GEMM_TILE", cfg)
        L.load().vb_tune_reload()
        v, r = eng.forward(inp["x_latent"], t_idx, cond, seed=11, return_routes=True)
        torch.cuda.synchronize()
        outs.append((v.clone(), r.clone()))
    monkeypatch.delenv("VB_GEMM_TILE")
    L.load().vb_tune_reload()
    for other in outs[1:]:
        assert torch.equal(outs[0][1], other[1])
        assert torch.equal(outs[0][0], other[0])


def test_small_tile_selection_is_bit_identical(engines, monkeypatch):
    """The launcher takes 64 x 64 tiles when a launch would make fewer than VB_GEMM_SMALL_TILES (200) tiles of 128 x 128 (one or two
    clips); VB_GEMM_SMALL=0 keeps the 128 x 128 kernel, VB_GEMM_SMALL_TILES=100000 sends every launch to the small tiles: all three
    selections must give the same bits (a clip's result must not depend on the batch-driven tile choice)."""
    eng = engines[(4, "bf16")]
    T, Lc = 752, 80
    inp = clip_batch(1, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2,), 321, dtype=torch.int64)
    outs = []
    for env in ({}, {"VB_GEMM_SMALL": "0"}, {"VB_GEMM_SMALL_TILES": "100000"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L.load().vb_tune_reload()
        v_, r_ = eng.forward(inp["x_latent"], t_idx, cond, seed=11, return_routes=True)
        torch.cuda.synchronize()
        outs.append((v_.clone(), r_.clone()))
        for k in env:
            monkeypatch.delenv(k)
    L.load().vb_tune_reload()
    for other in outs[1:]:
        assert torch.equal(outs[0][1], other[1]) and torch.equal(outs[0][0], other[0])


def test_p8_p16_projections_are_bit_identical(engines, monkeypatch):
    """Round 4: from two clips up the QKV + RoPE and routed-SwiGLU launches run on the 8-wave 256 x 256 kernel with the P16 column layout
    (gemm_bf16_p8_kernel<.., 32, 5, 0, 0, 2>); VB_GEMM_P8_OFF=1 keeps the 4-wave 128 x 128 kernels.  Both walk K in the same MFMA order
    and share the epilogue arithmetic: outputs and routes must be bit-identical, in both precisions - and since one clip (too few tiles
    for the 8-wave kernel) always takes the 4-wave path, a clip's bits keep not depending on the batch it rides in."""
    T, Lc = 752, 80
    t_idx = torch.full((8,), 321, dtype=torch.int64)
    for prec in ("bf16", "split"):
        eng = engines[(4, prec)]
        inp = clip_batch(4, T, Lc)
        cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
        outs = []
        for off in (False, True):
            if off:
                monkeypatch.setenv("VB_GEMM_P8_OFF", "1")
            L.load().vb_tune_reload()
            v, r = eng.forward(inp["x_latent"], t_idx, cond, seed=11, return_routes=True)
            torch.cuda.synchronize()
            outs.append((v.clone(), r.clone()))
        monkeypatch.delenv("VB_GEMM_P8_OFF")
        L.load().vb_tune_reload()
        assert torch.equal(outs[0][1], outs[1][1]), prec
        assert torch.equal(outs[0][0], outs[1][0]), describe(f"8-wave P16 vs 4-wave projections ({prec})", outs[0][0], outs[1][0])
        # clip 0 alone (4-wave small tiles) == clip 0 of the batch of four (8-wave kernel)
        inp1 = clip_batch(1, T, Lc)
        cond1 = eng.precompute_cond(torch.cat([inp1["t5_cond"], inp1["t5_uncond"]]), inp1["midi"], inp1["beats"], T)
        v1 = eng.forward(inp1["x_latent"], t_idx[:2], cond1, seed=11)
        torch.cuda.synchronize()
        assert torch.equal(v1[0], outs[0][0][0]), f"{prec}: clip 0 depends on its batch"


needs_experiments = pytest.mark.skipif(not (torch.cuda.is_available() and L.load().vb_has_experiments()),
                                       reason="kernel exists in the experiments build only (VB_BUILD_EXPERIMENTS=1 python -m versband_amd.build)")


@needs_experiments
def test_eight_wave_gemm_matches_four_wave_kernels(engines, monkeypatch):
    """The launcher takes the 8-wave 256x256 ping-pong kernel for large problems and the 4-wave kernels for small ones (one clip):
    both walk K in the same MFMA order and share the epilogue code, so every epilogue of the DiT (QKV+RoPE, gated residual, fp32
    scores, grouped SwiGLU with row gather, row-scatter / scatter-add) must give bit-identical outputs and routes."""
    B, T, Lc = 4, 752, 80
    inp = clip_batch(B, T, Lc)
    t_idx = torch.full((2 * B,), 321, dtype=torch.int64)
    for prec in ("bf16", "split"):
        eng = engines[(4, prec)]
        cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
        outs = []
        # "1+p16": the 8-wave kernel with the P16 column layout on the QKV + RoPE (epilogue 2) and SwiGLU (4) launches (prepared at the end
        # of round 3 for the first A/B of round 4, tools/gpu_ab_p8_p16.sh)
        for p8 in ("0", "1", "1+p16"):
            monkeypatch.setenv("VB_GEMM_P8", p8[0])
            if p8.endswith("p16"):
                monkeypatch.setenv("VB_GEMM_P8_P16", str((1 << 2) | (1 << 4)))
            L.load().vb_tune_reload()
            v, r = eng.forward(inp["x_latent"], t_idx, cond, seed=11, return_routes=True)
            torch.cuda.synchronize()
            outs.append((v.clone(), r.clone()))
        monkeypatch.delenv("VB_GEMM_P8")
        monkeypatch.delenv("VB_GEMM_P8_P16")
        L.load().vb_tune_reload()
        for k in (1, 2):
            assert torch.equal(outs[0][1], outs[k][1]), (prec, k)
            assert torch.equal(outs[0][0], outs[k][0]), describe(f"8-wave vs 4-wave GEMM ({prec}, form {k})", outs[k][0], outs[0][0])


@pytest.mark.parametrize("E,B,T", [(4, 2, 752), (4, 4, 752), (4, 5, 700), (8, 3, 752), (8, 4, 700)])
def test_fused_band_experts_match_two_gemm_path(ctx, sds, engines, monkeypatch, E, B, T):
    """bf16 production mode runs the band experts as ONE launch (w1/w3 -> SwiGLU -> w2, hidden kept in LDS; 192-channel bands at
    4 experts, 96-channel bands at 8); it walks K in the same order as the two grouped GEMMs and uses their epilogue arithmetic, so
    the results must be bit-identical.
    The fused kernel runs where cdiv(N, tile rows) * E >= 128 (band_fused_eligible in dit.hip; N = 2 B T token rows, 192 rows per tile
    at E = 4, 256 at E = 8):
      (4, 2, 752)  N = 3008: 16 tiles x 4 = 64 - NOT fused, both runs take the two-GEMM path (kept: the small-batch rule itself)
      (4, 4, 752)  N = 6016: 32 x 4 = 128 - fused, 192-channel kernel, the last tile has 64 rows
      (4, 5, 700)  N = 7000: 37 x 4 = 148 - fused, the last tile has 88 rows, four blocks of the grid return early
      (8, 3, 752)  N = 4512: 18 x 8 = 144 - fused, 96-channel kernel, the last tile has 160 rows
      (8, 4, 700)  N = 5600: 22 x 8 = 176 - fused, the last 256-row tile has 224 rows"""
    from versband_amd.engine import DiTEngine
    eng = engines[(4, "bf16")] if E == 4 else DiTEngine(ctx, synth.DiTConfig(num_experts=8), sds[8], precision="bf16")
    Lc = 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 777, dtype=torch.int64)
    v1, r1 = eng.forward(inp["x_latent"], t_idx, cond, seed=4, return_routes=True)
    torch.cuda.synchronize()
    v1, r1 = v1.clone(), r1.clone()
    monkeypatch.setenv("VB_BAND_UNFUSED", "1")
    L.load().vb_tune_reload()
    v2, r2 = eng.forward(inp["x_latent"], t_idx, cond, seed=4, return_routes=True)
    torch.cuda.synchronize()
    monkeypatch.delenv("VB_BAND_UNFUSED")
    L.load().vb_tune_reload()
    assert torch.equal(r1, r2)
    assert torch.equal(v1, v2), describe("fused vs two-GEMM band experts", v1, v2)


@pytest.mark.parametrize("B,T,mode", [(4, 752, "1"), (3, 700, "1"), (8, 752, "1"), (8, 752, "2"), (4, 752, "3")])
def test_single_launch_routed_w2_matches_two_launch_path(engines, sds, monkeypatch, B, T, mode):
    """bf16 production mode at >= 4096 token rows runs the second product of BOTH routed expert groups as ONE plain GEMM over
    (caption, acoustic) pair buckets (moe_w2_pair_kernel: K = 2H; the gate weights m_c / m_a are folded into the hidden rows by the
    SwiGLU epilogue before their bf16 rounding) instead of scatter-fp32 + scatter-add.  Same mathematics, one rounding placed
    differently (bf16(m h) against m * bf16(h)): the DiT output must agree with the two-launch path (VB_W2_PAIR=0) to bf16 rounding
    noise, block 0 must route identically (its routing does not see the change), and both stay equally close to the fp32 oracle.
    VB_W2_PAIR=2 / 3 force the 128 x 128 / 128 x 192 tile (ragged pair buckets at T = 700)."""
    eng = engines[(4, "bf16")]
    Lc = 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 555, dtype=torch.int64)
    assert 2 * B * T >= 4096
    monkeypatch.setenv("VB_W2_PAIR", mode)
    L.load().vb_tune_reload()
    v1, r1 = eng.forward(inp["x_latent"], t_idx, cond, seed=9, return_routes=True)
    torch.cuda.synchronize()
    v1, r1 = v1.clone(), r1.clone()
    monkeypatch.setenv("VB_W2_PAIR", "0")
    L.load().vb_tune_reload()
    v2, r2 = eng.forward(inp["x_latent"], t_idx, cond, seed=9, return_routes=True)
    torch.cuda.synchronize()
    monkeypatch.delenv("VB_W2_PAIR")
    L.load().vb_tune_reload()
    assert torch.isfinite(v1).all()
    assert torch.equal(r1[0], r2[0]), "block 0 routes must not depend on how w2 is launched"
    flips = float((r1 != r2).float().mean())
    err = rel_l2(v1, v2)
    print(f"pair w2 (mode {mode}) vs two launches: rel_l2 {err:.3e}, route flips {flips:.2e}")
    assert err < 2e-3 and flips < 1e-3, describe("single-launch pair w2 vs two launches", v1, v2)
    if B == 4 and mode == "1":
        # against the fp32 oracle on the same device-drawn noise: both forms are bf16 evaluations of the same sums
        noise = [tuple(torch.from_numpy(np.concatenate([prng.device_router_exponentials(9, c, 0, br, blk, gate, T, w) for c in range(B)]))
                       for gate, w in ((0, 2), (1, 4), (2, 4))) for br in (0, 1) for blk in range(4)]
        sd = sds[4]
        for br, key in ((0, "t5_cond"), (1, "t5_uncond")):
            c = ref_cpu.dit_precompute(sd, inp[key], inp["midi"], inp["beats"], T)
            ref = ref_cpu.dit_forward(sd, inp["x_latent"], t_idx[:B], c, noise[br * 4:(br + 1) * 4])
            e1, e2 = rel_l2(v1[br * B:(br + 1) * B], ref), rel_l2(v2[br * B:(br + 1) * B], ref)
            print(f"  branch {br}: vs oracle pair {e1:.3e}, two-launch {e2:.3e}")
            assert e1 < 5e-3 and e1 < 1.5 * e2 + 1e-4


@pytest.mark.parametrize("knob", ["VB_PROJ_IN_CONV", "VB_FINAL_GEMM"])
@pytest.mark.parametrize("prec,B,T,nb", [("bf16", 2, 752, 2), ("split", 3, 700, 2), ("split", 2, 333, 1)])
def test_proj_in_as_gemm_matches_the_conv_launch(engines, monkeypatch, prec, B, T, nb, knob):
    """proj_in (Conv1d 20 -> 768, k = 5) runs as im2col + split-precision GEMM with the bias / acoustic add in the epilogue and the row
    written for both CFG branches; VB_PROJ_IN_CONV=1 restores the conv launch.  Both are fp32-class evaluations of the same 100-term
    sums in another order: the DiT output agrees to fp32 rounding noise and the routes are identical (conditional-only batches too).
    Same for the FinalLayer: one wave per token row (LayerNorm + modulate in registers, exact-fp32 768 x 20 projection against LDS-resident
    weights) against the split-planes kernel + MFMA GEMM it replaced (VB_FINAL_GEMM=1)."""
    eng = engines[(4, prec)]
    Lc = 80
    inp = clip_batch(B, T, Lc)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]) if nb == 2 else inp["t5_cond"]
    cond = eng.precompute_cond(t5, inp["midi"], inp["beats"], T)
    t_idx = torch.full((nb * B,), 77, dtype=torch.int64)
    v1, r1 = eng.forward(inp["x_latent"], t_idx, cond, seed=5, return_routes=True)
    torch.cuda.synchronize()
    v1, r1 = v1.clone(), r1.clone()
    monkeypatch.setenv(knob, "1")
    L.load().vb_tune_reload()
    v2, r2 = eng.forward(inp["x_latent"], t_idx, cond, seed=5, return_routes=True)
    torch.cuda.synchronize()
    monkeypatch.delenv(knob)
    L.load().vb_tune_reload()
    err = rel_l2(v1, v2)
    print(f"{knob} off vs on ({prec}): rel_l2 {err:.3e}, route flips {int((r1 != r2).sum())}")
    assert torch.isfinite(v1).all()
    assert err < (2e-3 if prec == "bf16" else 2e-5), describe("proj_in as GEMM vs conv launch", v1, v2)
    assert int((r1 != r2).sum()) <= (4 if prec == "bf16" else 0)


@pytest.mark.parametrize("B,T", [(2, 752), (3, 100)])
def test_vae_wide_convs_as_gemm_match_the_conv_kernel(ctx, monkeypatch, B, T):
    """The VAE's wide layers (>= 384 output channels, pre-activated transposed planes as input) run as tap-by-tap GEMMs on the DMA-fed
    128 x 128 kernel (split precision, bias + residual in a channel-major epilogue); VB_CONV_GEMM_OFF=1 restores the conv kernel.
    Both are bf16x3 evaluations of the same sums in another order: decoder outputs agree to fp32 rounding noise (ragged tiles: T = 100)."""
    from versband_amd.engine import build_vae_decoder
    sdv = synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1)
    vae = build_vae_decoder(ctx, sdv)
    z = torch.from_numpy(prng.normal(77, B * 20 * T)).float().reshape(B, 20, T)
    m1 = vae.run(z).clone()
    torch.cuda.synchronize()
    monkeypatch.setenv("VB_CONV_GEMM_OFF", "1")
    L.load().vb_tune_reload()
    m2 = vae.run(z).clone()
    torch.cuda.synchronize()
    monkeypatch.delenv("VB_CONV_GEMM_OFF")
    L.load().vb_tune_reload()
    err = rel_l2(m1, m2)
    print(f"VAE decode, wide convs as GEMM vs conv kernel: rel_l2 {err:.3e}")
    assert torch.isfinite(m1).all() and err < 2e-5, describe("VAE wide convs as GEMM", m1, m2)
    ref = ref_cpu.vae_decode(sdv, z)
    assert rel_l2(m1, ref) < 2e-4, describe("VAE decode vs oracle", m1, ref)


@pytest.mark.parametrize("knob", ["VB_QKV_P16_OFF", "VB_QKV_VT16_OFF", "VB_RMSNORM_GENERIC", "VB_NO_XCD_GROUPS", "VB_BIG_TILE_MIN_K=0", "VB_WIDE_RESID=0",
                                  "VB_BAND_EPI_OLD"])
@pytest.mark.parametrize("prec,B,T", [("bf16", 4, 752), ("split", 3, 700), ("bf16", 1, 752), ("bf16", 8, 752)])
def test_qkv_p16_column_layout_is_bit_identical(engines, monkeypatch, prec, B, T, knob):
    """The QKV + RoPE GEMM fills its weight tile with permuted source rows so a lane's accumulator holds 16 CONSECUTIVE output columns
    (16-byte q / k stores and RoPE-table loads instead of 8-byte ones): the same values in other lanes - the DiT output must not change
    by a bit against the quad layout (VB_QKV_P16_OFF=1), in both precisions, full and ragged row tiles.  Same for the XCD-affine
    tile order of the per-clip grouped caption-gate GEMM (VB_NO_XCD_GROUPS=1 restores the interleaved order): same tiles, other CUs;
    the K >= 384 rule of the 192 x 192 kernel (VB_BIG_TILE_MIN_K=0) and the 128 x 192 gated-residual kernel at 8 clips (VB_WIDE_RESID=0): same k order, other tiles."""
    eng = engines[(4, prec)]
    Lc = 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 123, dtype=torch.int64)
    v1, r1 = eng.forward(inp["x_latent"], t_idx, cond, seed=3, return_routes=True)
    torch.cuda.synchronize()
    v1, r1 = v1.clone(), r1.clone()
    kname, _, kval = knob.partition("=")
    monkeypatch.setenv(kname, kval or "1")
    L.load().vb_tune_reload()
    v2, r2 = eng.forward(inp["x_latent"], t_idx, cond, seed=3, return_routes=True)
    torch.cuda.synchronize()
    monkeypatch.delenv(kname)
    L.load().vb_tune_reload()
    assert torch.isfinite(v1).all() and torch.equal(r1, r2)
    assert torch.equal(v1, v2), describe("P16 vs quad column layout of the QKV epilogue", v1, v2)


@pytest.mark.parametrize("knob", ["VB_ROUTER_GENERIC", "VB_ROUTER_TPW=4", "VB_ROUTER_TPW=1", "VB_ROUTER_GENERIC=1 VB_ROUTER_TPW=4"])
@pytest.mark.parametrize("E,prec,B,T", [(4, "bf16", 4, 752), (4, "bf16", 1, 752), (4, "split", 3, 700), (8, "split", 4, 752), (8, "split", 1, 300)])
def test_router_forms_are_bit_identical(engines, monkeypatch, E, prec, B, T, knob):
    """The router kernel runs two tokens per wave with the score columns per lane (10 = 80 keys x 8 heads / 64) and the expert count as
    compile-time constants; the run-time-bound form (VB_ROUTER_GENERIC), four tokens per wave (VB_ROUTER_TPW=4, rounds 1-2) and one
    (the small-launch form) must choose the same routes and gate weights to the bit: same additions in the same order."""
    eng = engines[(E, prec)]
    Lc = 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 321, dtype=torch.int64)
    v1, r1 = eng.forward(inp["x_latent"], t_idx, cond, seed=5, return_routes=True)
    torch.cuda.synchronize()
    v1, r1 = v1.clone(), r1.clone()
    names = []
    for kv in knob.split():
        kname, _, kval = kv.partition("=")
        monkeypatch.setenv(kname, kval or "1")
        names.append(kname)
    L.load().vb_tune_reload()
    v2, r2 = eng.forward(inp["x_latent"], t_idx, cond, seed=5, return_routes=True)
    torch.cuda.synchronize()
    for kname in names:
        monkeypatch.delenv(kname)
    L.load().vb_tune_reload()
    assert torch.isfinite(v1).all() and torch.equal(r1, r2)
    assert torch.equal(v1, v2), describe("router forms", v1, v2)


@needs_experiments
@pytest.mark.parametrize("E,B,T", [(4, 4, 752), (4, 6, 500), (8, 4, 752)])
def test_fused_score_router_matches_two_launches(ctx, sds, engines, monkeypatch, E, B, T):
    """The opt-in fused caption-gate kernel (VB_SCORE_FUSED=1, score_router.hip: a workgroup owns 64 tokens x all 640 score columns,
    the scores stay in LDS, the router's own device code runs on them; measured slower than the two launches, kept as an experiment).
    Same k-order, same bias add, same router code: routes, gate weights and the DiT output must be bit-identical to the grouped
    score GEMM + router kernel, for full and ragged last tiles (T = 500 = 7 x 64 + 52), with injected and device noise."""
    from versband_amd.engine import DiTEngine
    eng = engines[(4, "bf16")] if E == 4 else DiTEngine(ctx, synth.DiTConfig(num_experts=8), sds[8], precision="bf16")
    Lc = 80
    inp = clip_batch(B, T, Lc)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 413, dtype=torch.int64)
    noise = gumbel_arrays([exp_noise(B, T, E, 0, 4), exp_noise(B, T, E, 1, 4)]) if E == 4 and T == 752 else None
    runs = []
    for fused in (True, False):
        if fused:
            monkeypatch.setenv("VB_SCORE_FUSED", "1")
        else:
            monkeypatch.delenv("VB_SCORE_FUSED")
        L.load().vb_tune_reload()
        out = []
        for kw in ([dict(seed=21)] + ([dict(noise=noise)] if noise is not None else [])):
            v, r = eng.forward(inp["x_latent"], t_idx, cond, return_routes=True, **kw)
            torch.cuda.synchronize()
            out.append((v.clone(), r.clone()))
        runs.append(out)
    L.load().vb_tune_reload()
    for (v1, r1), (v2, r2) in zip(*runs):
        assert torch.isfinite(v1).all()
        assert torch.equal(r1, r2), f"routes differ at {(r1 != r2).sum().item()} of {r1.numel()} decisions"
        assert torch.equal(v1, v2), describe("fused score + router vs two launches", v1, v2)


def test_fullsize_reference_digests(ctx, engines):
    """BASELINE geometry (one 20 s clip: T = 752, L = 80, T_mel = 1504) against digests of the REFERENCE's own outputs
    (tests/golden/fullsize_digests.npz): DiT forward in split precision on injected noise, VAE decode, VAE encode, HiFi-GAN."""
    from versband_amd.engine import build_hifigan, build_vae_decoder, build_vae_encoder
    g = np.load(os.path.join(GOLD, "fullsize_digests.npz"))
    B, T, Lc, E = 1, 752, 80, 4
    inp = clip_batch(B, T, Lc)
    eng = engines[(E, "split")]
    cond = eng.precompute_cond(inp["t5_cond"], inp["midi"], inp["beats"], T)
    v = eng.forward(inp["x_latent"], torch.from_numpy(g["dit_t_idx"]), cond, noise=gumbel_arrays([exp_noise(B, T, E, 0, 4)]))
    torch.cuda.synchronize()
    check_digest(v, g, "dit_v_", 1e-4)
    vcfg, hcfg = synth.VAEConfig(), synth.HifiGanConfig()
    z = torch.from_numpy(synth.prng.normal(synth.prng.key_seed(SEED, "full_z"), 20 * T).reshape(1, 20, T))
    mel = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(vcfg), SEED + 1)).run(z)
    check_digest(mel, g, "vae_mel_", 2e-4)
    mom = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(vcfg), SEED + 3)).run(mel)
    check_digest(mom, g, "vae_moments_", 4e-4)
    wav = build_hifigan(ctx, synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2), hcfg.as_hparams()).run(mel)
    torch.cuda.synchronize()
    check_digest(wav, g, "voc_wav_", 1e-3)
    # the exact-fp32 VAE / vocoder (round 4: what bench.py's `value` runs) at the same geometry, against the same digests of the reference:
    # DMA-fed f32-MFMA kernels incl. the small tiles one clip selects, nearest x2 under DMA, per-clip weights (VAE attention), fused fp32 pairs
    mel32 = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(vcfg), SEED + 1), precision="fp32").run(z)
    check_digest(mel32, g, "vae_mel_", 2e-6)       # measured: sampled error 1.5e-6 of max-abs, L2 6.7e-8 (split: 1.0e-5 / 4.0e-7)
    mom32 = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(vcfg), SEED + 3), precision="fp32").run(mel32)
    check_digest(mom32, g, "vae_moments_", 2e-5)
    wav32 = build_hifigan(ctx, synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2), hcfg.as_hparams(), precision="fp32").run(mel32)
    torch.cuda.synchronize()
    check_digest(wav32, g, "voc_wav_", 2e-6)       # measured: 1.2e-6 / 1.7e-8 (split: 7.5e-6 / 1.4e-6)
    # fp32 with F(2,3) minimal filtering (round 6, conv1d_f32w.hip: the VAE's 3-tap layers, the generator's 64 / 128 / 256-channel ResBlock
    # convolutions - its 64-channel pairs run as two minimal-filtering launches, the 32-channel pairs fused with minimal filtering in both
    # convolutions, respair_f32w.hip): fp32 products, ~1.45x fewer; held to the SAME bounds against the reference's own outputs as the direct
    # fp32 kernels
    melmf = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(vcfg), SEED + 1), precision="fp32mf").run(z)
    check_digest(melmf, g, "vae_mel_", 2e-6)
    wavmf = build_hifigan(ctx, synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2), hcfg.as_hparams(), precision="fp32mf").run(melmf)
    torch.cuda.synchronize()
    check_digest(wavmf, g, "voc_wav_", 2e-6)
    mommf = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(vcfg), SEED + 3), precision="fp32mf").run(melmf)
    check_digest(mommf, g, "vae_moments_", 2e-5)
    assert not torch.equal(wavmf, wav32)                 # (the mode really took the other kernels)
    print(f"fp32mf vs fp32 direct at full size: mel max|d| {float((melmf - mel32).abs().max()):.3e} of {float(mel32.abs().max()):.3f}, "
          f"wav max|d| {float((wavmf - wav32).abs().max()):.3e} of {float(wav32.abs().max()):.3f}")


def test_t5_encoder_vs_transformers_golden_and_oracle(ctx):
    """T5 text encoder through vb_t5_encode (split-precision GEMMs, fp32 attention with the relative-position bias)
    against transformers.T5EncoderModel fixtures (2 layers: slice + digest, 24 layers: digest) and the oracle on a ragged length."""
    from versband_amd.engine import T5Engine
    g = np.load(os.path.join(GOLD, "t5_encode.npz"))
    sd = synth.make_state_dict(synth.t5_encoder_shapes(synth.T5Config(vocab_size=512, num_layers=2)), SEED + 5)
    enc = T5Engine(ctx, sd)
    out = enc.encode(torch.from_numpy(g["ids"]))
    torch.cuda.synchronize()
    assert rel_l2(out[:, :, :48], g["out_slice"]) < 1e-4, describe("t5 vs transformers", out[:, :, :48], g["out_slice"])
    check_digest(out, g, "out_", 1e-4)
    ids = torch.from_numpy((synth.prng.uniform(99, 3 * 37, 0.0, 1.0) * 512).astype(np.int64).reshape(3, 37)).clamp(0, 511)
    ref = ref_cpu.t5_encode(sd, ids)
    out = enc.encode(ids)
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < 1e-4, describe("t5 L=37 vs oracle", out, ref)
    sd24 = synth.make_state_dict(synth.t5_encoder_shapes(synth.T5Config(vocab_size=2048)), SEED + 5)
    out24 = T5Engine(ctx, sd24).encode(torch.from_numpy(g["ids24"]))
    torch.cuda.synchronize()
    check_digest(out24, g, "out24_", 3e-4)


@pytest.mark.parametrize("tag", ["amp1", "amp2"])
@pytest.mark.parametrize("prec,tol", [("fp32", 5e-5), ("fp32mf", 5e-5), ("split", 3e-4)])
def test_bigvgan_vs_golden_and_oracle(ctx, tag, prec, tol):
    """BigVGAN generator (anti-aliased Snake / SnakeBeta kernel + the shared conv kernels) against the reference's
    own outputs and, on a ragged length, against the oracle."""
    from tests.test_oracle_golden import _BV_CFGS
    from versband_amd.engine import build_bigvgan
    g = np.load(os.path.join(GOLD, "bigvgan.npz"))
    cfg = synth.BigVGANConfig(**_BV_CFGS[tag])
    sd = synth.make_state_dict(synth.bigvgan_shapes(cfg), SEED + 7)
    net = build_bigvgan(ctx, sd, cfg.as_hparams(), precision=prec)
    wav = net.run(torch.from_numpy(g[tag + "_mel"]))
    torch.cuda.synchronize()
    assert rel_l2(wav, g[tag + "_wav"]) < tol, describe("bigvgan vs reference", wav, g[tag + "_wav"])
    mel = torch.from_numpy(synth.prng.uniform(31, 2 * 80 * 37, -5.0, 1.5).reshape(2, 80, 37))
    ref = ref_cpu.bigvgan_forward(sd, cfg.as_hparams(), mel)
    wav = net.run(mel)
    torch.cuda.synchronize()
    assert wav.shape == ref.shape
    assert rel_l2(wav, ref) < tol, describe("bigvgan T=37 vs oracle", wav, ref)


def test_full_size_properties(ctx, engines):
    """BASELINE geometry (T=752, L=80): size-independent checks - finite outputs, CFG with scale 1 equals the
    conditional-only path, padding frames beyond T never leak (Tpad masking), full-length VAE/vocoder shapes."""
    eng = engines[(4, "bf16")]
    B, T, Lc = 2, 752, 80
    inp = clip_batch(B, T, Lc)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]])
    cond2 = eng.precompute_cond(t5, inp["midi"], inp["beats"], T)
    idx, dts = vm.euler_tables(3)
    x2 = eng.sample_cfg(inp["x_latent"], cond2, idx, dts, 1.0, seed=9)
    cond1 = eng.precompute_cond(inp["t5_cond"], inp["midi"], inp["beats"], T)
    x1 = eng.sample_cfg(inp["x_latent"], cond1, idx, dts, 1.0, seed=9)
    torch.cuda.synchronize()
    assert torch.isfinite(x2).all()
    # e_u + 1*(e_c - e_u) == e_c up to fp32 rounding of the guidance arithmetic
    assert rel_l2(x2, x1) < 1e-5, describe("scale=1 CFG vs cond-only", x2, x1)
    from versband_amd.engine import build_hifigan, build_vae_decoder
    sdv = synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1)
    mel = build_vae_decoder(ctx, sdv).run(x2)
    assert mel.shape == (B, 80, 2 * T) and torch.isfinite(mel).all()
    hcfg = synth.HifiGanConfig()
    sdh = synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2)
    wav = build_hifigan(ctx, sdh, hcfg.as_hparams()).run(mel[:1])
    torch.cuda.synchronize()
    assert wav.shape == (1, 1, 2 * T * 320) and torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0


# ---------------------------------------------------------------- log-mel front-end
def _test_audio(B, n, seed):
    """seeded clip: a few drifting partials + noise, louder than full scale in places (the clamp must act)"""
    t = np.arange(n, dtype=np.float64) / 24000.0
    out = []
    for b in range(B):
        f0 = 110.0 * (b + 2)
        y = sum(0.3 / (k + 1) * np.sin(2 * np.pi * f0 * (k + 1) * t * (1.0 + 0.01 * np.sin(2 * np.pi * 0.3 * t))) for k in range(6))
        y = 1.6 * y * (0.6 + 0.9 * np.sin(2 * np.pi * 0.5 * t) ** 2) + 0.05 * synth.prng.normal(seed + b, n)
        out.append(y)
    return torch.from_numpy(np.stack(out).astype(np.float32))


def test_melnet_vs_golden_and_oracle():
    """MelNet on the HIP library (frames kernel -> fp32 MFMA hop-block convolution -> mel tail) against the reference's own MelNet
    outputs (tests/golden/melnet.npz) and, at BASELINE length (20 s, 1500 frames) and on ragged / centred inputs, the oracle."""
    from tests.test_oracle_golden import MEL_HP, mel_close
    from versband_amd._lib import VersbandError
    from versband_amd.melnet import MelNet
    g = np.load(os.path.join(GOLD, "melnet.npz"))
    net = MelNet(MEL_HP)
    with pytest.raises(VersbandError):
        net(torch.zeros(1, 6400))                       # no CPU path
    net.to("cuda:0")
    assert np.abs(net.mel_basis.cpu().numpy() - g["mel_basis"]).max() <= 1e-8       # two independent restatements of the filterbank
    fb = net.mel_basis.cpu()
    for tag, tol in (("a", 1e-5), ("b", 1e-2), ("c", 1e-5)):
        out = net(torch.from_numpy(g["wav_" + tag]))
        torch.cuda.synchronize()
        mel_close(out.cpu().numpy(), g["mel_" + tag], tol)
    # numpy 1-D input, like the reference accepts
    out = net(g["wav_c"][0])
    mel_close(out.cpu().numpy(), g["mel_c"], 1e-5)
    # BASELINE length, 3 clips (odd batch), 20 s + a ragged tail
    wav = _test_audio(3, 1500 * 320 + 77, 77)
    assert float(wav.abs().max()) > 1.0
    out = net(wav)
    torch.cuda.synchronize()
    ref = ref_cpu.melnet_forward(wav, MEL_HP, fb)
    assert out.shape == ref.shape == (3, 80, 1500) and net.frames(wav.shape[1]) == 1500
    mel_close(out.cpu().numpy(), ref.numpy(), 1e-3)
    # torch.stft(center=True) geometry
    short = wav[:2, :40 * 320]
    outc = net(short, center=True)
    refc = ref_cpu.melnet_forward(short, MEL_HP, fb, center=True)
    assert outc.shape == refc.shape == (2, 80, 44)
    mel_close(outc.cpu().numpy(), refc.numpy(), 1e-3)
    # complex spectrum [B, T, n_fft/2+1, 2]
    sp = net(short, complex=True)
    y = torch.nn.functional.pad(short.clamp(-1, 1).unsqueeze(1), [480, 480], mode="reflect").squeeze(1)
    fr = y.unfold(-1, 1280, 320).double() * torch.hann_window(1280).double()
    rs = torch.view_as_real(torch.fft.rfft(fr, dim=-1))
    assert sp.shape == rs.shape == (2, 40, 641, 2)
    assert float((sp.cpu().double() - rs).abs().max()) <= 1e-5 * float(rs.abs().max())
    # loud failure on an input shorter than the reflect padding
    with pytest.raises(ValueError):
        net(torch.zeros(1, 300))


def test_melnet_closes_the_loop_on_the_vocoder(ctx):
    """Harness-level use (scripts/test_final.py --eval_mel): the mel of a vocoded clip has the frame count of the mel that was
    vocoded, is finite and sits above the log floor - the shape contract `mel L1 against real audio` relies on."""
    from versband_amd.engine import build_hifigan
    from tests.test_oracle_golden import MEL_HP
    from versband_amd.melnet import MelNet
    hcfg = synth.HifiGanConfig()
    sdh = synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2)
    mel = torch.from_numpy(synth.prng.uniform(5, 2 * 80 * 64, -4.0, 0.5).reshape(2, 80, 64).astype(np.float32))
    wav = build_hifigan(ctx, sdh, hcfg.as_hparams()).run(mel)
    back = MelNet(MEL_HP, device="cuda:0")(wav[:, 0])
    torch.cuda.synchronize()
    assert back.shape == mel.shape and torch.isfinite(back).all() and float(back.min()) >= -5.0
