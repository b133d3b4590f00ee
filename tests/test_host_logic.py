"""CPU tests of the host logic: packing layouts, Euler/t-index tables, factory + checkpoint plumbing."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from versband_amd import model as vm
from versband_amd import pack, prng, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prng_is_stable():
    # exact values: the uniform pipeline is integer arithmetic and must never drift across machines
    u = prng.uniform(prng.key_seed(1234, "x"), 4)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    assert prng.bits64(1, 2).tolist() == [10451216379200822465, 13757245211066428519]
    e = prng.exponential(5, 1000)
    assert (e > 0).all() and abs(float(e.mean()) - 1.0) < 0.1


def test_planes_split_is_fp32_class():
    w = torch.from_numpy(prng.normal(3, 4096)).reshape(64, 64)
    p2 = pack.to_planes(w, 2)
    assert p2.dtype == torch.bfloat16 and p2.shape == (2, 64, 64)
    assert float((pack.planes_to_float(p2) - w).abs().max() / w.abs().max()) < 2 ** -15
    assert torch.equal(pack.to_planes(w, 1)[0], p2[0])


def test_conv_transpose_polyphase_packing_matches_conv_transpose():
    for (ci, co, k, u) in [(3, 2, 16, 8), (2, 3, 15, 5), (2, 2, 11, 5), (1, 1, 4, 2)]:
        w = torch.from_numpy(prng.normal(9, ci * co * k).reshape(ci, co, k)).double()
        x = torch.from_numpy(prng.normal(10, ci * 13).reshape(1, ci, 13)).double()
        p = (k - u) // 2
        ref = F.conv_transpose1d(x, w, stride=u, padding=p)
        wp = pack.pack_conv_transpose(w.float(), u).double()
        kmax = wp.shape[1]
        out = torch.zeros_like(ref)
        T_out = ref.shape[-1]
        for ph in range(u):                     # restates the kernel's polyphase index arithmetic
            d = p - ph
            q0 = (d + u - 1) // u if d > 0 else 0
            in_off, out_off = q0 - (kmax - 1), q0 * u + ph - p
            n = 0
            while n * u + out_off < T_out:
                acc = torch.zeros(co, dtype=torch.float64)
                for j in range(kmax):
                    idx = n + in_off + j
                    if 0 <= idx < x.shape[-1]:
                        acc += wp[ph, j].T @ x[0, :, idx]
                out[0, :, n * u + out_off] = acc
                n += 1
        assert torch.allclose(out, ref, atol=1e-12), (ci, co, k, u)


def test_euler_tables_match_oracle_and_quirk():
    for n in (10, 24, 50):
        idx, dts = vm.euler_tables(n + 1)
        _, ref = ref_cpu.t_index_table(n + 1)
        assert idx == ref and len(dts) == n
        assert abs(sum(dts) - 1.0) < 1e-5
    idx, _ = vm.euler_tables(51)
    assert idx[5] == 99 and idx[9] == 179             # float32 truncation quirk
    idx, dts = vm.euler_tables(25, t_start=20)
    assert len(idx) == 4


def test_pack_dit_layouts():
    cfg = synth.DiTConfig()
    sd = synth.make_state_dict(synth.dit_shapes(cfg), 1)
    pk = pack.pack_dit(sd, cfg, 2, "cpu")
    b0 = pk["blocks"][0]
    D, H, E = cfg.hidden_size, cfg.ffn_hidden, cfg.num_experts
    assert b0["wqkv"].shape == (2, 3 * D, D) and b0["w13"].shape == (2, 2 * E, 2 * H, D) and b0["w2"].shape == (2, 2 * E, D, H)
    assert b0["w13f"].shape == (2, E, 2 * H, D // E) and b0["w2f"].shape == (2, E, D // E, H)
    w13 = pack.planes_to_float(b0["w13"])
    assert torch.allclose(w13[1, 0::2], sd["blocks.0.feed_forward.caption_experts.1.w1.weight"], atol=1e-6)
    assert torch.allclose(w13[E + 2, 1::2], sd["blocks.0.feed_forward.acoustic_experts.2.w3.weight"], atol=1e-6)
    w2f = pack.planes_to_float(b0["w2f"])
    band = D // E
    assert torch.allclose(w2f[3], sd["blocks.0.feed_forward.freq_experts.3.w2.weight"][3 * band:4 * band], atol=1e-6)
    assert pk["top"]["adaln_w"].shape == (cfg.depth * 6 * D + 2 * D, D)
    assert torch.equal(pk["top"]["t_freq_table"][416], ref_cpu.timestep_embedding(torch.tensor([416]))[0])
    assert torch.allclose(b0["cross_w"], torch.tanh(sd["blocks.0.attention.gate"]))
    # out_proj folded into the caption gate: same logits as the two chained linears
    a = torch.from_numpy(prng.normal(5, 7 * D)).reshape(7, D)
    p0 = "blocks.0.feed_forward."
    chained = F.linear(F.linear(a, sd[p0 + "cross_attention.out_proj.weight"], sd[p0 + "cross_attention.out_proj.bias"]),
                       sd[p0 + "caption_gating_network.weight"], sd[p0 + "caption_gating_network.bias"])
    assert torch.allclose(F.linear(a, b0["wcg"], b0["bcg"]), chained, atol=2e-6)


def test_factory_and_checkpoint_plumbing(tmp_path):
    cfg = vm.load_config(os.path.join(ROOT, "configs", "vocal2music.yaml"))
    m = vm.instantiate_from_config(cfg.model)
    assert type(m).__name__ == "CFM" and m.first_stage_model.embed_dim == 20 and m.num_timesteps == 1000
    assert m.model.diffusion_model.cfg.ffn_hidden == 512
    with pytest.raises(KeyError):
        vm.instantiate_from_config({"params": {}})
    sd = {"model.diffusion_model." + k: v for k, v in synth.make_state_dict(synth.dit_shapes(synth.DiTConfig()), 1).items()}
    sd["scale_factor"] = torch.tensor(0.5)
    sd["betas"] = torch.zeros(1000)                        # DDPM buffers are ignored like strict=False does
    m.load_state_dict(sd, strict=False)
    assert float(m.scale_factor) == 0.5 and "proj_in.weight" in m._dit_state
    s = vm.CFMSampler(m, num_timesteps=1000)
    assert s._shape([20, 752], 8) == (8, 20, 752)
    assert s._shape(None, 2) == (2, 20, 750)
    # get_learned_conditioning passes pre-computed T5 embeddings through and keeps the acoustic dict
    c = m.get_learned_conditioning({"caption": torch.zeros(2, 80, 1024), "acoustic": {"midi": 1}, "name": ["a", "b"]})
    assert c["caption"].shape == (2, 80, 1024) and c["acoustic"] == {"midi": 1}
    # text captions without T5 weights / tokenizer: loud failure (the reference would fail in from_pretrained), never silent noise
    with pytest.raises(RuntimeError, match="dummy_text"):
        m.get_learned_conditioning({"caption": ["Style: pop", ""], "acoustic": {}, "name": ["a", "b"]})
    m.cond_stage_model.dummy_text = True                   # explicit opt-in (cond_stage_config params / --dummy_text)
    c = m.get_learned_conditioning({"caption": ["Style: pop", ""], "acoustic": {}, "name": ["a", "b"]})
    assert c["caption"].shape == (2, 80, 1024)
    c2 = m.get_learned_conditioning({"caption": ["Style: pop", ""], "acoustic": {}, "name": ["a", "b"]})
    assert torch.equal(c["caption"], c2["caption"]) and not torch.equal(c["caption"][0], c["caption"][1])
    # .to(device) reaches the text encoder too (one GPU per process, scripts/test_final.py initialize_model)
    m.to("cuda:3")
    assert str(m.cond_stage_model.device) == "cuda:3"
    m.to("cpu")


def test_vocoder_checkpoint_discovery(tmp_path):
    import yaml
    hcfg = synth.HifiGanConfig()
    base = tmp_path / "base.yaml"
    yaml.safe_dump({"resblock": "2", "upsample_initial_channel": 512}, open(base, "w"))
    hp = hcfg.as_hparams()
    hp["base_config"] = "./base.yaml"
    yaml.safe_dump(hp, open(tmp_path / "config.yaml", "w"))
    got = vm.set_hparams(str(tmp_path / "config.yaml"))
    assert got["resblock"] == "1" and got["upsample_rates"] == [8, 5, 4, 2]        # child overrides base
    torch.save({"state_dict": {"model_gen.conv_pre.bias": torch.ones(3), "model_disc.x": torch.ones(1)}},
               tmp_path / "model_ckpt_steps_20.ckpt")
    torch.save({"state_dict": {"model_gen.conv_pre.bias": torch.zeros(3)}}, tmp_path / "model_ckpt_steps_3.ckpt")
    sd = vm.load_ckpt_state(str(tmp_path))
    assert list(sd) == ["conv_pre.bias"] and float(sd["conv_pre.bias"].sum()) == 3.0


def test_synthetic_inputs_respect_embedding_ranges():
    c = synth.make_clip_inputs(1234, 3, 752)
    assert c["midi"].shape == (1, 1504) and int(c["midi"].max()) <= 128 and int(c["beats"].max()) <= 2
    assert int(c["midi"][0, -1]) == 128 and int(c["beats"][0, -1]) == 2               # pad values
    a, b = synth.make_clip_inputs(1234, 3, 16), synth.make_clip_inputs(1234, 4, 16)
    assert not torch.equal(a["x_latent"], b["x_latent"])


def test_longform_window_plan_and_crossfade_partition_of_unity():
    from versband_amd import longform
    assert longform.plan_windows(700, 1500, 128) == [(0, 700)]
    plan = longform.plan_windows(4500, 1500, 128)
    assert plan[0] == (0, 1500) and plan[-1][0] + plan[-1][1] == 4500 and all(n == 1500 for _, n in plan)
    covered = torch.zeros(4500)
    for s, n in plan:
        covered[s:s + n] += 1
    assert covered.min() >= 1
    # cross-fading constant windows gives back the constant (weights sum to one everywhere)
    parts = [torch.full((2, 3, n), 7.0) for _, n in plan]
    out = longform.crossfade_windows(parts, plan, 4500)
    assert torch.allclose(out, torch.full((2, 3, 4500), 7.0), atol=1e-6)
    # a window's interior (outside every overlap) is passed through untouched
    parts = [torch.full((1, 1, n), float(i)) for i, (_, n) in enumerate(plan)]
    out = longform.crossfade_windows(parts, plan, 4500)
    assert float(out[0, 0, 200]) == 0.0 and float(out[0, 0, plan[1][0] + 700]) == 1.0


# ---------------------------------------------------------------- harness I/O
def _write_manifest(tmp_path, rows):
    cols = ["name", "duration", "caption", "key", "key_confidence", "avg_pitch", "tempo", "tempo_confidence", "emotion", "wav_len",
            "mel_path", "vocal_mel_path", "audio_path"]
    p = tmp_path / "total.tsv"
    with open(p, "w") as f:
        f.write("\t".join(cols) + "\n")
        for r in rows:
            f.write("\t".join(str(r[c]) for c in cols) + "\n")
    return str(p)


def _make_items(tmp_path, lengths, vocal_lengths=None, durations=None):
    rows, midi, beats = [], {}, {}
    rs = np.random.RandomState(0)
    for i, T in enumerate(lengths):
        name = f"song{i:02d}"
        np.save(tmp_path / f"{name}_mel.npy", rs.uniform(-5, 1, (80, T)).astype(np.float32))
        Tv = (vocal_lengths or lengths)[i]
        np.save(tmp_path / f"{name}_vocal_mel.npy", rs.uniform(-5, 1, (80, Tv)).astype(np.float32))
        midi[name] = rs.randint(0, 129, T)
        beats[name] = rs.randint(0, 2, T)
        rows.append(dict(name=name, duration=(durations or [T / 75.0] * len(lengths))[i], caption="warm pop<psep>soft rock", key="C major",
                         key_confidence=0.9, avg_pitch=60.0, tempo=100.0, tempo_confidence=0.8, emotion="['happy', 'calm', 'bright']",
                         wav_len=T / 75.0, mel_path=str(tmp_path / f"{name}_mel.npy"), vocal_mel_path=str(tmp_path / f"{name}_vocal_mel.npy"),
                         audio_path=str(tmp_path / f"{name}_accomp.wav")))
    np.save(tmp_path / "midi.npy", midi, allow_pickle=True)
    np.save(tmp_path / "beats.npy", beats, allow_pickle=True)
    return _write_manifest(tmp_path, rows), str(tmp_path / "midi.npy"), midi, beats


def test_infer_dataset_items(tmp_path):
    """scripts/test_final.py:196-340: lengths round up to 8 frames, acoustic = first 20 vocal-mel rows padded with -5, midi / beats
    cropped to the mel and padded with 0, captions 'Style: .. Musical: ..', items longer than 20 s dropped, corrupted inputs replaced."""
    from versband_amd.harness import InferDataset
    manifest, midi_path, midi, beats = _make_items(tmp_path, [301, 750, 1600, 200], vocal_lengths=[301, 752, 1600, 120],
                                                   durations=[4.0, 10.0, 21.3, 2.7])
    ds = InferDataset(manifest, midi_path, seed=3)
    assert len(ds) == 3 and sorted(i["name"] for i in ds.items) == ["song00", "song01", "song03"]     # song02 is > 20 s
    by_name = {ds.items[i]["name"]: ds[i] for i in range(len(ds))}
    a = by_name["song00"]
    assert a["acoustic"].shape == (20, 304) and a["image"].shape == (80, 304) and a["midi"].shape == a["beats"].shape == (1, 304)
    vm_ = np.load(tmp_path / "song00_vocal_mel.npy")
    assert torch.equal(a["acoustic"][:, :301], torch.from_numpy(vm_[:20])) and float(a["acoustic"][:, 301:].max()) == -5.0
    assert torch.equal(a["midi"][0, :301].long(), torch.from_numpy(midi["song00"]).long()) and float(a["midi"][0, 301:].abs().max()) == 0.0
    assert torch.equal(a["beats"][0, :301].long(), torch.from_numpy(beats["song00"]).long())
    assert float(a["image"][:, 301:].max()) == -5.0 and a["audio_path"].endswith("song00_accomp.wav")
    assert a["caption"].startswith("Style: ") and " Musical: " in a["caption"] and a["ori_caption"] in ("Style: warm pop ", "Style: soft rock ")
    b = by_name["song01"]            # vocal mel 2 frames longer than the mel: cropped to the mel length, then rounded up to 752
    assert b["acoustic"].shape == (20, 752) and torch.equal(b["acoustic"][:, :750], torch.from_numpy(np.load(tmp_path / "song01_vocal_mel.npy")[:20, :750]))
    c = by_name["song03"]            # vocal mel 80 frames short: declared corrupted -> pad values 128 / 2 / -5 (:282-286)
    assert c["acoustic"].shape == (20, 200) and float(c["acoustic"].max()) == -5.0
    assert float(c["midi"].min()) == 128.0 and float(c["beats"].min()) == 2.0
    os.remove(tmp_path / "song00_mel.npy")      # unreadable mel: 75 frames of floor (:270-277) -> the vocal mel no longer matches
    d = ds[[i for i in range(len(ds)) if ds.items[i]["name"] == "song00"][0]]
    assert d["image"].shape == (80, 80) and float(d["image"].max()) == -5.0
    with pytest.raises(FileNotFoundError):
        InferDataset(str(tmp_path / "missing.tsv"), midi_path)


def test_caption_generator_rules():
    """Decision rules of CaptionGenerator2 (caption_generator.py:781-837, :612-670): confidence gates, dead zones, key naming."""
    import random
    from versband_amd.harness import CaptionGenerator2
    g = CaptionGenerator2(random.Random(0))
    assert g.prepare_tempo(100, 0.2) is None and g.prepare_tempo(0, 0.9) is None
    assert g.prepare_tempo(60, 0.9) == "very slow" and g.prepare_tempo(170, 0.9) == "very fast"
    assert g.prepare_tempo(70, 0.9) is None and g.prepare_tempo(90, 0.9) is None and g.prepare_tempo(160, 0.9) is None     # dead zones
    assert g.prepare_tempo(100, 0.9) in ("medium", "moderate") and g.prepare_tempo(130, 0.9) in ("fast", "quick")
    assert g.prepare_avg_pitch(50) in ("low", "relatively low") and g.prepare_avg_pitch(54) is None and g.prepare_avg_pitch(80) == "very high"
    assert g.prepare_avg_pitch(-1) is None and g.prepare_avg_pitch(63) is None and g.prepare_avg_pitch(70) in ("high", "relatively high")
    assert g.prepare_key("C major", 0.4) is None and g.prepare_key("None", 0.9) is None
    assert {g.prepare_key("C major", 0.9) for _ in range(40)} == {"C major", "A minor"}
    assert {g.prepare_key("f#", 0.9) for _ in range(40)} == {"F-sharp minor", "A major"}
    assert {g.prepare_key("B-", 0.9) for _ in range(40)} == {"B-flat major", "G minor"}
    assert g.prepare_emotion([]) is None and g.prepare_emotion(["sad"]) == "sad"
    e3 = g.prepare_emotion(["a", "b", "c"])
    assert e3.count(", ") == 2 and ", and " in e3 and sorted(e3.replace(", and ", ", ").split(", ")) == ["a", "b", "c"]
    durs = {g.prepare_duration(12.2) for _ in range(40)}
    assert durs == {"a long time", "12 seconds"} and {g.prepare_duration(5.0) for _ in range(40)} == {None, "5 seconds"}
    full = g.transcribe(key="G major", key_conf=0.9, avg_pitch=70, tempo=130, tempo_conf=0.9, emotion=["tense"], duration=18.0)
    assert full.startswith("The melody is in ") and "pitch" in full and "tempo" in full and full.endswith("It carries a tense mood.")
    assert g.transcribe() == "" and g.transcribe(emotion=["calm"]) == "It carries a calm mood."


def test_wav_and_tsv_round_trip(tmp_path):
    from versband_amd.harness import load_samples_from_tsv, pad_or_cut_xd, read_wav, save_rows_to_tsv, write_wav_pcm16
    t = np.arange(2400) / 24000.0
    wav = 0.5 * np.sin(2 * np.pi * 440 * t)
    wav[:3] = [1.5, -1.5, 0.999999]                                       # clipping
    p = str(tmp_path / "sub" / "a[0][accomp].wav")
    write_wav_pcm16(p, wav, 24000)
    back, sr = read_wav(p)
    assert sr == 24000 and back.shape == wav.shape and back.dtype == np.float64
    assert back[0] == 32767 / 32768 and back[1] == -1.0 and np.abs(back[3:] - wav[3:]).max() <= 0.5 / 32768 + 1e-12
    rows = [{"audio_path": p, "caption": "Style: pop Musical: The melody is in C major.", "name": "x"}, {"audio_path": "q", "caption": "", "name": "y"}]
    save_rows_to_tsv(rows, ["audio_path", "caption", "name"], tmp_path / "clap.csv")
    assert load_samples_from_tsv(tmp_path / "clap.csv") == rows
    x = np.arange(12).reshape(2, 6)
    assert pad_or_cut_xd(x, 4, 1).tolist() == [[0, 1, 2, 3], [6, 7, 8, 9]] and pad_or_cut_xd(x, 8, 1, -5)[0].tolist() == [0, 1, 2, 3, 4, 5, -5, -5]
    xt = pad_or_cut_xd(torch.ones(2, 3), 5, dim=1, pad_value=2.0)
    assert torch.is_tensor(xt) and xt.shape == (2, 5) and xt[0].tolist() == [1, 1, 1, 2, 2]


def test_reference_import_paths_of_the_mel_front_end():
    from preprocess.NAT_mel import MelNet
    from versband_amd import melnet
    assert MelNet is melnet.MelNet
    net = MelNet(dict(fft_size=1280, audio_num_mel_bins=80, audio_sample_rate=24000, hop_size=320, win_size=1280, fmin=0, fmax=8000))
    assert net.mel_basis.shape == (80, 641) and net.hann_window.shape == (1280,) and net.frames(480000) == 1500 and net.frames(480000, center=True) == 1504
    with pytest.raises(ValueError):
        MelNet(dict(fft_size=1024, audio_num_mel_bins=80, audio_sample_rate=24000, hop_size=300, win_size=1024, fmin=0, fmax=8000))


def test_entry_script_keeps_the_reference_cli(monkeypatch):
    """Every flag of the reference's scripts/test_final.py:34-98 parses here with the same type (defaults differ only where the
    reference hard-codes paths of its authors' machines)."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("vb_test_final", os.path.join(ROOT, "scripts", "test_final.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["test_final.py", "--config", "c.yaml", "--ckpt", "m.ckpt", "--manifest_path", "t.tsv", "--other_condition",
                                      "midi.npy", "--ddim_steps", "50", "--n_samples", "2", "--scale", "2.5", "--scales", "1-2-3", "--save_dir", "out",
                                      "--save_plot", "--num_gpus", "4", "--sample_rate", "24000"])
    a = mod.parse_args()
    assert (a.config, a.ckpt, a.manifest_path, a.other_condition) == ("c.yaml", "m.ckpt", "t.tsv", "midi.npy")
    assert (a.ddim_steps, a.n_samples, a.scale, a.scales, a.save_dir, a.save_plot, a.num_gpus, a.sample_rate) == (50, 2, 2.5, "1-2-3", "out", True, 4, 24000)
    monkeypatch.setattr(sys, "argv", ["test_final.py"])
    d = mod.parse_args()
    assert d.scales == "1-3" and d.scale == 3.0 and d.n_samples == 1 and d.save_dir == "test" and d.num_gpus == 1 and d.sample_rate == 24000


def test_bench_line_is_one_short_json_line():
    """Round 5's bench line grew to 21 KB and the driver recorded `parsed: null`.  The stdout line is built by
    bench.compact_line() from the full result dict: <= 4 KB, one `{...}` line, every contract key + `roofline` + `cpu_baseline`
    present; the tables go to the side file it names.  Canned input: the committed round-5 result (profiles/r05_final_bench_c2.json),
    once as is and once inflated (8 ranks, long strings) to prove the limit holds by construction."""
    import copy
    import json
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_final_bench_c2.json")))
    assert len(json.dumps(full)) > 15000                     # the canned dict IS the oversized one
    big = copy.deepcopy(full)
    big["n_gpus"] = 8
    big["ranks"].update({"world": 8, "backend": "nccl (RCCL)", "weight_broadcast_ms": 123.456789, "weight_broadcast_gbps": 45.678901,
                         "per_rank_ms": [139.391012518] * 8})
    big["config"]["workload"] = big["config"]["workload"] * 3
    big["cpu_baseline"]["sample"] = big["cpu_baseline"]["sample"] * 5
    r06 = json.load(open(os.path.join(ROOT, "profiles", "r06_f_bench_detail.json")))     # three timed regions: value (fp32mf), fp32_direct, split
    assert "fp32_direct" in r06 and "direct_equivalent" in r06["roofline"]
    for src in (full, big, r06):
        s = bench.compact_line(src, "/tmp/bench_detail.json")
        assert len(s) <= bench.LINE_MAX == 4096 and "\n" not in s and s.startswith("{") and s.endswith("}")
        d = json.loads(s)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                  "config", "parity_check", "roofline", "cpu_baseline", "detail"):
            assert k in d, k
        assert d["metric"] == src["metric"] and d["unit"] == "mel-s/s" and d["n_gpus"] == src["n_gpus"]
        assert abs(d["value"] - src["value"]) <= 1e-5 * src["value"] and abs(d["ms_per_step"] - src["ms_per_step"]) <= 1e-5 * src["ms_per_step"]
        assert "workload" in d["config"] and "model" not in d["config"]
        rf = d["roofline"]
        for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us", "path_frac"):
            assert k in rf, k
        assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
        cb = d["cpu_baseline"]
        assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "mel-s/s" and cb["sample"]
        assert d["parity_check"]["ok"] is True and d["parity_check"]["worst"]["latent_rel_l2"] < 1e-3
    d6 = json.loads(bench.compact_line(r06, None))
    assert d6["fp32_direct"]["parity_ok"] is True and d6["split"]["parity_ok"] is True and d6["value"] > d6["fp32_direct"]["value"]
    assert d6["roofline"]["direct_equivalent"]["frac"] > d6["roofline"]["frac"] and d6["config"]["vocoder_precision"] == "fp32mf"
    d8 = json.loads(bench.compact_line(big, None))
    assert d8["ranks"]["backend"] == "nccl (RCCL)" and len(d8["ranks"]["per_rank_ms"]) == 8 and d8["detail"] is None
    # a result without the optional blocks (--no-parity-check --no-cpu-baseline --no-isolated) still makes a line
    bare = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                 "dtype", "data", "config")}
    bare["roofline"] = {"bound": "mfma", "kernel": "k", "achieved": 1.0, "peak": 2.0, "unit": "TFLOP/s", "frac": 0.5, "traffic": None}
    bare["parity_check"] = None
    assert json.loads(bench.compact_line(bare, None))["roofline"]["frac"] == 0.5


def test_bench_plain_run_options_and_output_dump(tmp_path):
    """A plain `bench.py` run times the K steps and prints the contract keys only; --full adds the rest.  --dump-outputs writes float32
    .npy files of at most 64 MB in all, the same elements on every run (c3's 32 clips do not fit whole: the waveform is sampled)."""
    import json
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full and a.dump_outputs == str(tmp_path)
    for bad in (["--steps", "0"], ["--profile-timed"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)
    rng = np.random.default_rng(5)
    arrays = {"latent": rng.standard_normal((32, 20, 752)), "mel": rng.standard_normal((32, 80, 1504)).astype(np.float32),
              "wav": rng.standard_normal((32, 1, 481280)).astype(np.float32)}
    runs = []
    for d in (tmp_path / "a", tmp_path / "b"):
        shapes = bench.dump_outputs(arrays, str(d))
        assert shapes["latent"] == (32, 20, 752) and shapes["mel"] == (32, 80, 1504) and len(shapes["wav"]) == 1
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6
        runs.append({n: np.load(d / f"{n}.npy") for n in arrays})
    for n in arrays:
        assert runs[0][n].dtype == np.float32 and np.array_equal(runs[0][n], runs[1][n]), n
    assert np.array_equal(runs[0]["latent"], arrays["latent"].astype(np.float32))
    assert np.isin(runs[0]["wav"], arrays["wav"].reshape(-1)).all()
    plain = {"metric": "m", "value": 1.5, "unit": "mel-s/s", "n_gpus": 1, "steps": 7, "warmup": 3, "ms_per_step": 2.0, "higher_is_better": True,
             "scaling": "weak", "vs_baseline": None, "dtype": "d", "data": "x", "config": {"workload": "w"}}
    d = json.loads(bench.compact_line(plain, None))
    assert d["ms_per_step"] == 2.0 and d["steps"] == 7 and "roofline" not in d and "parity_check" not in d


def _model_keys(tree, prefix=""):
    out = set()
    if isinstance(tree, dict):
        for k, v in tree.items():
            out.add(prefix + k)
            out |= _model_keys(v, prefix + k + ".")
    return out


def _check_boundary_config(path):
    """load_config -> instantiate_from_config(config.model) -> CFMSampler(model, 1000), the three calls of
    scripts/test_final.py initialize_model (reference :137-150), then the attributes the harness reads."""
    import warnings
    cfg = vm.load_config(path)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = vm.instantiate_from_config(cfg.model)
    assert type(m).__name__ == "CFM"
    assert m.num_timesteps == 1000 and (m.mel_dim, m.mel_length, m.channels) == (20, 750, 0)
    assert m.first_stage_model.embed_dim == 20 and m.first_stage_model.ddconfig["ch_mult"] == [1, 2, 4]
    assert m.cond_stage_model.max_length == 80
    c = m.model.diffusion_model.cfg
    assert (c.hidden_size, c.depth, c.num_heads, c.max_len, c.num_experts, c.context_dim) == (768, 4, 8, 1500, 4, 768)
    assert m.model.conditioning_key == "hybrid"
    s = vm.CFMSampler(m, 1000)
    assert s.num_timesteps == 1000 and s._shape(None, 3) == (3, 20, 750)
    return cfg, [str(x.message) for x in w]


def test_full_key_config_takes_the_reference_constructor_paths():
    """configs/vocal2music_full.yaml (travels to the GPU box) carries every key of the reference's `model:` tree, including the
    ones this path ignores and a dangling first-stage ckpt_path: same model as the trimmed config, a warning for the ckpt."""
    cfg, warns = _check_boundary_config(os.path.join(ROOT, "configs", "vocal2music_full.yaml"))
    assert any("ckpt_path" in x and "not found" in x for x in warns), warns
    for k in ("linear_start", "linear_end", "num_timesteps_cond", "log_every_t", "cond_stage_trainable", "monitor", "use_ema", "scheduler_config"):
        assert k in cfg.model.params, k
    assert "lightning" in cfg and "data" in cfg and "test_dataset" in cfg
    trimmed = vm.load_config(os.path.join(ROOT, "configs", "vocal2music.yaml"))
    assert trimmed.model.params.unet_config == cfg.model.params.unet_config
    assert trimmed.model.params.first_stage_config.params.ddconfig == cfg.model.params.first_stage_config.params.ddconfig
    assert trimmed.model.params.cond_stage_config == cfg.model.params.cond_stage_config


def test_reference_yaml_loads_unchanged(golden_dir, tmp_path):
    """"the YAML file loads unchanged".  The reference's own configs/vocal2music.yaml:1-128, held as digests
    (tests/golden/reference_config_digest.json, oracle/gen_golden.py:gen_config_digest): the committed full-key config must cover its
    every key, so the GPU box runs the same paths; the reference's tree rebuilt from those keys must equal it in every model value bar
    the checkpoint path, and go through the three calls of initialize_model."""
    import json
    import yaml
    from tests.helpers import config_hash, config_key_paths, config_restrict
    g = json.load(open(os.path.join(golden_dir, "reference_config_digest.json")))
    ours = yaml.safe_load(open(os.path.join(ROOT, "configs", "vocal2music_full.yaml")))
    by_hash = {config_hash(list(k)): k for k in config_key_paths(ours)}
    missing = set(g["key_paths"]) - set(by_hash)
    assert not missing, f"{len(missing)} key path(s) of the reference's config are not in configs/vocal2music_full.yaml"
    ref = config_restrict(ours, {by_hash[h] for h in g["key_paths"]})
    model = json.loads(json.dumps(ref["model"]))
    del model["params"]["first_stage_config"]["params"]["ckpt_path"]
    assert config_hash(model) == g["model_without_ckpt_path"]
    (tmp_path / "vocal2music.yaml").write_text(yaml.safe_dump(ref, sort_keys=False))
    cfg, warns = _check_boundary_config(str(tmp_path / "vocal2music.yaml"))
    assert any("ckpt_path" in x for x in warns)
    p = ours["model"]["params"]
    for k in ("unet_config", "cond_stage_config"):
        assert config_hash(p[k]) == g[k], k
    assert config_hash(p["first_stage_config"]["params"]["ddconfig"]) == g["first_stage_ddconfig"]


def test_oracle_long_form_restatement_matches_the_product_plan():
    """oracle/gen_bench_digest.py --long restates the window plan and the cross-fade itself (round 6: it imported them from the product
    package); the two restatements must agree - on the plan exactly, on the blend bit for bit."""
    import textwrap
    from versband_amd import longform
    src = open(os.path.join(ROOT, "oracle", "gen_bench_digest.py")).read()
    assert "from versband_amd.longform" not in src and "import versband_amd.longform" not in src
    i, j = src.index("    def plan_windows(T, window, overlap):"), src.index("    B, TL, WIN, OV = 4, 4500, 1500, 128")
    ns = {"torch": torch}
    exec(textwrap.dedent(src[i:j]), ns)
    for T, w, o in ((4500, 1500, 128), (1000, 1500, 128), (3000, 1500, 128), (1501, 1500, 128), (2872, 1500, 128), (6000, 1500, 0)):
        assert ns["plan_windows"](T, w, o) == longform.plan_windows(T, w, o)
    plan = longform.plan_windows(4500, 1500, 128)
    g = torch.Generator().manual_seed(3)
    parts = [torch.randn(2, 3, 1500, generator=g) for _ in plan]
    assert torch.equal(ns["crossfade_windows"](parts, plan, 4500), longform.crossfade_windows(parts, plan, 4500))
