"""HiFi-GAN with row lengths on the GPU (vb_hifigan_forward_lens, ConvNet.run(lengths=), HifiGAN.spec2wav_batch(lengths=)): mels of
different lengths as rows of one vocoder call.  The contract of include/versband_hip.h: row b's first len[b] * hop samples are the call on
that clip alone - bit for bit when len[b] and the padded T agree mod 4 (kernel routes depend on a length only through that residue), to
fp32 roundoff otherwise - the rest of the row is exact zeros, and the caller's mel padding is never read.

The generator is the synthetic one at upsample_initial_channel = 256: stages of 128 / 64 / 32 / 16 channels at 8 / 40 / 160 / 320 samples
per frame, so every precision runs unfused convolutions AND fused 64- / 32-channel pairs (fp32mf: 32 only).  Row ends fall inside the pair
kernels' output tiles at every stage (len * tmul is no multiple of a run length) and the short rows are shorter than one ring step.

One-frame rows: the float64 oracle takes T = 1 (every convolution pads), and so does the plain call in every precision - checked in
test_one_frame_clip_alone_runs_in_every_precision, which the one-frame batch of test (a) relies on.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, describe, rel_l2
from tests.test_bf16_mode import bf16_mode
from versband_amd import _lib as L
from versband_amd import harness, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("fp32", "fp32mf", "split", "bf16", "bf16xt")
CFG = synth.HifiGanConfig(upsample_initial_channel=256)
HOP = CFG.hop
# (a) / (b): every length agrees with T mod 4 - rows are bit-equal to the clip alone.  "one": a one-frame row beside a full one (1 = 5 mod 4)
SAME_RESIDUE = {"mod0": (24, [24, 20, 16, 12, 8, 4]), "mod2": (22, [22, 18, 10, 6, 2]), "one": (5, [5, 1])}
MIXED = (24, [24, 22, 13, 7])          # (c): residues 0, 2, 1, 3 under T = 24


@functools.lru_cache(maxsize=None)
def state():
    sd = synth.make_state_dict(synth.hifigan_shapes(CFG), SEED + 2)
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def mel_batch(T, B):
    """B rows of T frames, log-mel range; never modified (callers clone before they write padding)"""
    return torch.from_numpy(synth.prng.uniform(11, B * 80 * T, -5.0, 1.5).reshape(B, 80, T).copy())


def padded(T, lens, fill=0.0):
    mel = mel_batch(T, len(lens)).clone()
    for b, n in enumerate(lens):
        mel[b, :, n:] = fill
    return mel


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from versband_amd.engine import Context
    return Context("cuda:0")


@pytest.fixture(scope="module")
def nets(ctx):
    from versband_amd.engine import build_hifigan
    assert HOP == 320
    return {p: build_hifigan(ctx, state()[0], CFG.as_hparams(), precision=p) for p in PRECISIONS}


_cache = {}


def lens_run(nets, prec, T, lens):
    """the zero-padded call with lengths, once per (precision, batch): the reference of (a) and (b)"""
    key = (prec, T, tuple(lens))
    if key not in _cache:
        _cache[key] = nets[prec].run(padded(T, lens), lengths=lens).cpu()
    return _cache[key]


def alone(nets, prec, T, B, b, n):
    """the plain call on row b's clip alone"""
    return nets[prec].run(mel_batch(T, B)[b:b + 1, :, :n].contiguous()).cpu()


def test_program_has_unfused_convs_and_fused_pairs_of_both_widths(nets):
    for prec, net in nets.items():
        pairs = sorted({op.Ci for op in net.nb.ops if op.kind == L.OP_RESPAIR})
        convs = sorted({op.Ci for op in net.nb.ops if op.kind == L.OP_CONV and op.Ci == op.Co})
        assert pairs == ([32] if prec == "fp32mf" else [32, 64]), (prec, pairs)
        assert 128 in convs and 16 in convs, (prec, convs)


# ---------------------------------------------------------------------------------------------------------------- one-frame clips
@pytest.mark.parametrize("prec", PRECISIONS)
def test_one_frame_clip_alone_runs_in_every_precision(nets, prec):
    """what the one-frame row of (a) is compared with: the plain call at T = 1 against the float64 oracle, at the precision's bound"""
    mel = mel_batch(5, 2)[1:2, :, :1].contiguous()
    orc = _oracle(mel)
    wav = nets[prec].run(mel).cpu()
    assert wav.shape == orc[0].shape == (1, 1, HOP) and torch.isfinite(wav).all()
    _hold(prec, wav, orc, "one-frame clip alone")


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("name", list(SAME_RESIDUE))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_rows_equal_the_clip_alone_bit_for_bit(nets, prec, name):
    T, lens = SAME_RESIDUE[name]
    wav = lens_run(nets, prec, T, lens)
    assert wav.shape == (len(lens), 1, T * HOP)
    for b, n in enumerate(lens):
        ref = alone(nets, prec, T, len(lens), b, n)
        assert torch.equal(wav[b:b + 1, :, :n * HOP], ref), describe(f"{prec} {name}: row {b} (length {n} of {T}) vs the clip alone", wav[b:b + 1, :, :n * HOP], ref)
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0, f"{prec} {name}: row {b} has nonzero samples behind its end"
        assert torch.isfinite(wav[b]).all() and float(wav[b, :, :n * HOP].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("name", list(SAME_RESIDUE))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_padding_is_never_read(nets, prec, name, fill):
    T, lens = SAME_RESIDUE[name]
    wav = nets[prec].run(padded(T, lens, fill), lengths=lens).cpu()
    assert torch.isfinite(wav).all(), f"{prec} {name}: padding of {fill} reached the output"
    assert torch.equal(wav, lens_run(nets, prec, T, lens)), f"{prec} {name}: the result depends on the mel padding"


# ---------------------------------------------------------------------------------------------------------------- c
@functools.lru_cache(maxsize=None)
def oracle_row(b):
    """float64 oracle of row b of MIXED on the clip alone, and the bf16 mode's restatement of it (float64- and fp32-accumulated:
    tests/test_bf16_mode.py); computed once, never modified"""
    T, lens = MIXED
    return _oracle(mel_batch(T, len(lens))[b:b + 1, :, :lens[b]].contiguous())


def _oracle(mel):
    sd, sd64 = state()
    hp = CFG.as_hparams()
    ref = ref_cpu.hifigan_forward(sd64, hp, mel.double())
    with bf16_mode(torch.float64):
        r64 = ref_cpu.hifigan_forward(sd64, hp, mel.double())
    with bf16_mode(torch.float32):
        r32 = ref_cpu.hifigan_forward(sd, hp, mel.float())
    return ref, r64, rel_l2(r64, ref), rel_l2(r32, r64)


def _hold(prec, wav, orc, what):
    """wav [1][1][n] against orc = _oracle(the clip): the bound the suite holds that precision's vocoder to against the float64 oracle.  fp32 / fp32mf: rel-L2 <= 2e-5 and max-abs <=
    1e-4 x max|ref| (test_gpu_production.py); split: rel-L2 < 2e-4 (test_gpu_path.py::test_hifigan_vs_golden_and_oracle); bf16 / bf16xt:
    the two bounds of test_gpu_bf16_mode.py / test_gpu_bf16xt.py, with (a) and (b) of this clip - within 4 x (b) of the float64-accumulated
    restatement of the mode, within 1.25 x (a) of the oracle."""
    ref, r64, a, b = orc
    assert wav.shape == ref.shape
    e = rel_l2(wav, ref)
    if prec in ("fp32", "fp32mf"):
        am = float((wav.double() - ref).abs().max() / ref.abs().max())
        print(f"[{prec}] {what}: rel-L2 {e:.3e} (2e-5), max-abs / max|ref| {am:.3e} (1e-4)")
        assert e <= 2e-5 and am <= 1e-4, describe(f"{prec} {what} vs float64", wav, ref)
    elif prec == "split":
        print(f"[{prec}] {what}: rel-L2 {e:.3e} (2e-4)")
        assert e < 2e-4, describe(f"{prec} {what} vs float64", wav, ref)
    else:
        er = rel_l2(wav, r64)
        print(f"[{prec}] {what}: vs restatement {er:.3e} (4 x {b:.3e}), vs float64 {e:.3e} (1.25 x {a:.3e})")
        assert er < 4 * b, describe(f"{prec} {what} vs restatement", wav, r64)
        assert e < 1.25 * a, describe(f"{prec} {what} vs float64", wav, ref)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_mixed_residues_hold_the_precision_bound_like_the_clip_alone(nets, prec):
    T, lens = MIXED
    wav = nets[prec].run(padded(T, lens), lengths=lens).cpu()
    for b, n in enumerate(lens):
        assert oracle_row(b)[0].shape == (1, 1, n * HOP)
        _hold(prec, alone(nets, prec, T, len(lens), b, n), oracle_row(b), f"clip {b} alone (length {n})")
        _hold(prec, wav[b:b + 1, :, :n * HOP], oracle_row(b), f"row {b} of the lens call (length {n} of {T})")
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("prec", PRECISIONS)
def test_no_lengths_and_all_full_lengths_are_the_plain_call(nets, prec):
    net, B, T = nets[prec], 3, 24
    mel = mel_batch(T, B).cuda()
    plain = net.run(mel).cpu()
    assert torch.equal(net.run(mel, lengths=[T] * B).cpu(), plain)
    lib = net.ctx.lib
    ws = torch.empty(lib.vb_hifigan_lens_workspace_bytes(net.ctx.handle, B, T), dtype=torch.uint8, device="cuda")
    assert ws.numel() > lib.vb_net_workspace_bytes(net.ctx.handle, L.NET_VOCODER, B, T) + B * 80 * T * 4
    for lens in (None, L.Lens(None), L.Lens((C.c_int32 * B)(*[T] * B))):
        out = torch.full((B, 1, T * HOP), float("nan"), device="cuda")
        rc = lib.vb_hifigan_forward_lens(net.ctx.handle, L.ptr(mel), B, T, C.byref(lens) if lens is not None else None, L.ptr(out), L.ptr(ws), L.stream_ptr())
        assert rc == 0, lib.vb_last_error()
        assert torch.equal(out.cpu(), plain)


# ---------------------------------------------------------------------------------------------------------------- e
def test_refusals_name_the_row_or_the_limit_and_leave_wav_untouched(nets):
    net, T = nets["fp32mf"], 24
    lib = net.ctx.lib

    def call(lens):
        B = len(lens)
        mel = torch.zeros(B, 80, T, device="cuda")
        wav = torch.full((B, 1, T * HOP), 7.0, device="cuda")
        ws = torch.empty(max(256, lib.vb_hifigan_lens_workspace_bytes(net.ctx.handle, B, T)), dtype=torch.uint8, device="cuda")
        ls = L.Lens((C.c_int32 * B)(*lens))
        rc = lib.vb_hifigan_forward_lens(net.ctx.handle, L.ptr(mel), B, T, C.byref(ls), L.ptr(wav), L.ptr(ws), L.stream_ptr())
        torch.cuda.synchronize()
        assert bool((wav == 7.0).all()), "a refused call must not touch wav"
        return rc, lib.vb_last_error()

    rc, msg = call([24, 0, 12])
    assert rc == -1 and b"row 1" in msg and b"length 0" in msg
    rc, msg = call([24, 12, 25])
    assert rc == -1 and b"row 2" in msg and b"length 25" in msg
    rc, msg = call([12] * 65)
    assert rc == -1 and b"65 rows" in msg and b"1..64" in msg
    # the Python host states the same rules first, naming the caller's argument
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0"), ([24, 12, 25], r"lengths\[2\] = 25"), ([12] * 65, "65 rows")):
        with pytest.raises(ValueError, match=text):
            net.run(torch.zeros(len(lens), 80, T), lengths=lens)


def test_bigvgan_as_the_vocoder_is_refused_naming_the_op(ctx):
    from tests.test_bf16_mode import fixture_case
    from versband_amd.engine import build_bigvgan
    sd, cfg, x, _, _ = fixture_case("bigvgan_amp1")
    net = build_bigvgan(ctx, sd, cfg.as_hparams(), precision="fp32")
    assert net.which == L.NET_VOCODER
    B, _, T = x.shape
    first = next(i for i, op in enumerate(net.nb.ops) if op.kind == L.OP_AA_ACT)
    with pytest.raises(L.VersbandError) as e:
        net.run(torch.cat([x, x]), lengths=[T, T - 4])
    assert f"op {first} (VB_OP_AA_ACT)" in str(e.value) and "replicate-pad" in str(e.value)
    assert torch.equal(net.run(x, lengths=[T] * B), net.run(x))          # (full rows stay the plain call, whatever the program)


def test_vae_nets_raise_on_lengths(ctx):
    from versband_amd.engine import build_vae_decoder, build_vae_encoder
    dec = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1), precision="fp32")
    with pytest.raises(ValueError, match="VAE decoder"):
        dec.run(torch.zeros(2, dec.in_ch, 16), lengths=[16, 8])
    enc = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(synth.VAEConfig()), SEED + 3), precision="fp32")
    with pytest.raises(ValueError, match="VAE encoder"):
        enc.run(torch.zeros(2, enc.in_ch, 16 * enc.in_tmul), lengths=[16, 8])


# ---------------------------------------------------------------------------------------------------------------- f
def test_cli_vocoder_lengths_files_are_byte_identical(tmp_path):
    """scripts/infer_batched.py --items_per_batch 6 --length_slack 8 over items of 150, 152, 151, 153, 150, 154 latent tokens - mel lengths
    of both residues mod 4, so the group is vocoded in two calls with row lengths - against --length_slack 0: the same files byte for byte"""
    tokens = [150, 152, 151, 153, 150, 154]
    common = [sys.executable, os.path.join(ROOT, "scripts", "infer_batched.py"), "--synthetic", "6", "--synthetic_frames",
              ",".join(str(t * harness.MEL_DOWNSAMPLE) for t in tokens), "--ddim_steps", "2", "--scales", "3", "--n_samples", "1", "--items_per_batch", "6"]
    listing = {}
    for name, extra in (("slack", ["--length_slack", "8"]), ("none", ["--length_slack", "0"])):
        out = tmp_path / "gen"
        r = subprocess.run(common + extra + ["--save_dir", str(out)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {}
        for d, _, names in os.walk(out):
            for nm in names:
                if nm.endswith(".wav") or nm == "clap.csv":
                    p = os.path.join(d, nm)
                    files[os.path.relpath(p, out)] = open(p, "rb").read()
                    os.remove(p)
        listing[name] = files
    a, b = listing["slack"], listing["none"]
    assert sorted(a) == sorted(b) and len([f for f in a if f.endswith(".wav")]) == 6
    for name in sorted(a):
        assert a[name] == b[name], f"{name} differs between --length_slack 8 and --length_slack 0"
    calls = harness.plan_row_batches(tokens, [3.0], 1, 6, length_slack=8)
    assert len(calls) == 1 and calls[0]["row_lengths"] == tokens
    voc = harness.plan_vocoder_calls([2 * t for t in tokens])
    assert [c["rows"] for c in voc] == [[0, 1, 4, 5], [2, 3]] and all(c["lengths"] for c in voc)
