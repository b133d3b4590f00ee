"""VAE decoder with row lengths on the GPU (vb_vae_decode_lens, ConvNet.decode_lens, decode_first_stage(lengths=)): latents of different
lengths as rows of one decode call.  The contract of include/versband_hip.h: row b's first 2 * len[b] frames are vb_vae_decode on that clip
alone - bit for bit when len[b] and the padded T agree by the route rule (harness.DECODE_ROUTE_MOD), to the precision's roundoff otherwise -
the rest of the row is exact zeros, and neither the caller's latent padding nor anything in the workspace is read.

Two decoder programs in all five precisions: "wide" = VAEConfig() (384 / 768 / 1536 channels, cpg 12 / 24 / 48: the DMA-fed GEMM, gn_apply
and xt_planes routes, vectorised statistics) and "narrow" = VAEConfig(ch=32) (32 / 64 / 128 channels, cpg 1 / 2 / 4: GroupNorm inside the
register-staged convolutions and, at odd lengths, the scalar statistics path).  The attention block sits at the latent rate: its keys are
the row's tokens, so the 96- and 70-token sets run the softmax lane loop twice and their short rows end inside a tile at both time scales.
"""
import ctypes as C
import functools
import hashlib
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
CONFIGS = {"wide": synth.VAEConfig(), "narrow": synth.VAEConfig(ch=32)}
M = harness.DECODE_ROUTE_MOD
# every length agrees with T by the route rule: rows are bit-equal to the clip alone.  "r0" / "r2": more than 64 keys, short rows whose
# lengths are no multiple of 16 or 32 (the attention's channel counts); "one": a one-token row beside a full one
SAME_ROUTE = {"r0": (96, [96, 68, 36, 4]), "r2": (70, [70, 66, 38, 6, 2]), "one": (5, [5, 1])}
MIXED = (24, [24, 22, 13, 7, 1])          # every residue mod 4, odd lengths, a one-token row
ZC = 20


def test_the_sets_follow_the_documented_rule():
    assert M == 4
    for T, lens in SAME_ROUTE.values():
        assert all(n % M == T % M for n in lens) and lens[0] == T
        assert [c["rows"] for c in harness.plan_decode_calls(lens)] == [list(range(len(lens)))]
    assert {n % 4 for n in MIXED[1]} == {0, 1, 2, 3} and 1 in MIXED[1]


@functools.lru_cache(maxsize=None)
def state(cfg_name):
    sd = synth.make_state_dict(synth.vae_decoder_shapes(CONFIGS[cfg_name]), SEED + 1)
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def z_batch(T, B):
    """B latents of T tokens; never modified (callers clone before they write padding)"""
    return torch.from_numpy(synth.prng.normal(79, B * ZC * T).reshape(B, ZC, T).copy()).float()


def padded(T, lens, fill=0.0):
    z = z_batch(T, len(lens)).clone()
    for b, n in enumerate(lens):
        z[b, :, n:] = fill
    return z


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from versband_amd.engine import Context
    return Context("cuda:0")


@pytest.fixture(scope="module")
def nets(ctx):
    from versband_amd.engine import build_vae_decoder
    return {(c, p): build_vae_decoder(ctx, state(c)[0], precision=p) for c in CONFIGS for p in PRECISIONS}


_cache = {}


def lens_run(nets, cfg, prec, T, lens):
    """the zero-padded call with lengths, once per (program, precision, batch): the reference of checks 1 to 4"""
    key = (cfg, prec, T, tuple(lens))
    if key not in _cache:
        _cache[key] = nets[(cfg, prec)].decode_lens(padded(T, lens), lens).cpu()
    return _cache[key]


def alone(nets, cfg, prec, T, B, b, n):
    """the plain call on row b's clip alone"""
    return nets[(cfg, prec)].run(z_batch(T, B)[b:b + 1, :, :n].contiguous()).cpu()


def test_programs_contain_the_routes_the_shapes_are_meant_for(nets):
    for prec in PRECISIONS:
        wide, narrow = nets[("wide", prec)].nb.ops, nets[("narrow", prec)].nb.ops
        assert any(op.kind in (L.OP_GN_APPLY, L.OP_XT_PLANES) for op in wide) or prec == "bf16", prec
        assert any(op.kind == L.OP_CONV and op.stats >= 0 for op in narrow) or prec in ("fp32", "fp32mf"), prec
        assert any(op.kind == L.OP_SOFTMAX_T for op in wide) and any(op.kind == L.OP_GN_STATS for op in narrow)
    # between them the precisions cover gn_apply, xt_planes and GroupNorm inside the staged convolutions of both programs
    kinds = {(c, op.kind) for (c, _), net in nets.items() for op in net.nb.ops}
    assert ("wide", L.OP_GN_APPLY) in kinds and ("wide", L.OP_XT_PLANES) in kinds
    assert any(op.kind == L.OP_CONV and op.stats >= 0 for op in nets[("narrow", "split")].nb.ops)
    assert any(op.kind == L.OP_CONV and op.stats >= 0 for op in nets[("narrow", "bf16")].nb.ops)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(SAME_ROUTE))
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_rows_equal_the_clip_alone_bit_for_bit(nets, cfg, prec, name):
    T, lens = SAME_ROUTE[name]
    mel = lens_run(nets, cfg, prec, T, lens)
    assert mel.shape == (len(lens), 80, 2 * T)
    for b, n in enumerate(lens):
        ref = alone(nets, cfg, prec, T, len(lens), b, n)
        got = mel[b:b + 1, :, :2 * n]
        assert torch.equal(got, ref), describe(f"{cfg} {prec} {name}: row {b} (length {n} of {T}) vs the clip alone", got, ref)
        assert int(torch.count_nonzero(mel[b, :, 2 * n:])) == 0, f"{cfg} {prec} {name}: row {b} has nonzero frames behind its end"
        assert torch.isfinite(mel[b]).all() and float(got.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("name", list(SAME_ROUTE))
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_padding_is_never_read(nets, cfg, prec, name, fill):
    T, lens = SAME_ROUTE[name]
    mel = nets[(cfg, prec)].decode_lens(padded(T, lens, fill), lens).cpu()
    assert torch.isfinite(mel).all(), f"{cfg} {prec} {name}: padding of {fill} reached the output"
    assert torch.equal(mel, lens_run(nets, cfg, prec, T, lens)), f"{cfg} {prec} {name}: the result depends on the latent padding"


# ---------------------------------------------------------------------------------------------------------------- 3
def c_call(net, z, lens, ws_fill=None, out_fill=float("nan")):
    """vb_vae_decode_lens through the C ABI with a caller-owned workspace; returns (rc, message, mel on the host)"""
    lib = net.ctx.lib
    B, _, T = z.shape
    z = z.cuda().contiguous()
    ws = torch.empty(max(256, lib.vb_vae_decode_lens_workspace_bytes(net.ctx.handle, B, T)), dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    out = torch.full((B, 80, 2 * T), out_fill, device="cuda")
    rc = lib.vb_vae_decode_lens(net.ctx.handle, L.ptr(z), B, T, C.byref(lens) if lens is not None else None, L.ptr(out), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, lib.vb_last_error(), out.cpu()


@pytest.mark.parametrize("name", ["r2", "one"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_workspace_is_never_read(nets, cfg, prec, name):
    T, lens = SAME_ROUTE[name]
    net = nets[(cfg, prec)]
    outs = []
    for fill in (0xFF, 0x00):
        rc, msg, mel = c_call(net, padded(T, lens), L.Lens((C.c_int32 * len(lens))(*lens)), ws_fill=fill)
        assert rc == 0, msg
        assert torch.isfinite(mel).all(), f"{cfg} {prec} {name}: a workspace of {fill:#x} bytes reached the output"
        outs.append(mel)
    assert torch.equal(outs[0], outs[1]), describe(f"{cfg} {prec} {name}: 0xFF workspace vs zeroed", outs[0], outs[1])
    assert torch.equal(outs[0], lens_run(nets, cfg, prec, T, lens))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_rows_are_independent_of_their_neighbours(nets, cfg, prec):
    T, lens = SAME_ROUTE["r2"]
    base = lens_run(nets, cfg, prec, T, lens)
    z = padded(T, lens)
    other = list(lens)
    z[0] = z_batch(T, len(lens) + 1)[len(lens)]                  # another clip in row 0 ...
    other[0], other[2] = 33, 70                                   # ... of another length (and residue); row 2 grows to the full T
    z[0, :, 33:] = 0.0
    z[2] = z_batch(T, len(lens))[2]
    mel = nets[(cfg, prec)].decode_lens(z, other).cpu()
    for b in (1, 3, 4):
        assert torch.equal(mel[b], base[b]), describe(f"{cfg} {prec}: row {b} changed with its neighbours", mel[b], base[b])
    assert torch.equal(mel[2:3], alone(nets, cfg, prec, T, len(lens), 2, T))          # (row 2 is the full clip now)


# ---------------------------------------------------------------------------------------------------------------- 5
@functools.lru_cache(maxsize=None)
def oracle_row(cfg, b):
    """float64 oracle of row b of MIXED on the clip alone, and the bf16 mode's restatement of it (float64- and fp32-accumulated:
    tests/test_bf16_mode.py); computed once, never modified"""
    T, lens = MIXED
    z = z_batch(T, len(lens))[b:b + 1, :, :lens[b]].contiguous()
    sd, sd64 = state(cfg)
    ref = ref_cpu.vae_decode(sd64, z.double())
    with bf16_mode(torch.float64):
        r64 = ref_cpu.vae_decode(sd64, z.double())
    with bf16_mode(torch.float32):
        r32 = ref_cpu.vae_decode(sd, z.float())
    return ref, r64, rel_l2(r64, ref), rel_l2(r32, r64)


def _hold(prec, mel, orc, what):
    """mel [1][80][2n] against orc = oracle_row(...): the bound the suite holds that precision's VAE decoder to against the float64 oracle.
    fp32 / fp32mf: rel-L2 < 2e-5, split: < 2e-4 (tests/test_gpu_path.py::test_vae_decode_vs_golden_and_oracle, tests/golden/README.md);
    bf16 / bf16xt: the two bounds of test_gpu_bf16_mode.py / test_gpu_bf16xt.py with (a) and (b) of this clip - within 4 x (b) of the
    float64-accumulated restatement of the mode, within 1.25 x (a) of the oracle."""
    ref, r64, a, b = orc
    assert mel.shape == ref.shape
    e = rel_l2(mel, ref)
    if prec in ("fp32", "fp32mf", "split"):
        tol = 2e-4 if prec == "split" else 2e-5
        print(f"[{prec}] {what}: rel-L2 {e:.3e} ({tol:g})")
        assert e < tol, describe(f"{prec} {what} vs float64", mel, ref)
    else:
        er = rel_l2(mel, r64)
        print(f"[{prec}] {what}: vs restatement {er:.3e} (4 x {b:.3e}), vs float64 {e:.3e} (1.25 x {a:.3e})")
        assert er < 4 * b, describe(f"{prec} {what} vs restatement", mel, r64)
        assert e < 1.25 * a, describe(f"{prec} {what} vs float64", mel, ref)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_mixed_residues_hold_the_precision_bound_like_the_clip_alone(nets, cfg, prec):
    T, lens = MIXED
    mel = nets[(cfg, prec)].decode_lens(padded(T, lens), lens).cpu()
    for b, n in enumerate(lens):
        assert oracle_row(cfg, b)[0].shape == (1, 80, 2 * n)
        _hold(prec, alone(nets, cfg, prec, T, len(lens), b, n), oracle_row(cfg, b), f"{cfg} clip {b} alone (length {n})")
        _hold(prec, mel[b:b + 1, :, :2 * n], oracle_row(cfg, b), f"{cfg} row {b} of the lens call (length {n} of {T})")
        assert int(torch.count_nonzero(mel[b, :, 2 * n:])) == 0


# ---------------------------------------------------------------------------------------------------------------- 6
def _dev_lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


STATS_LENS = [70, 65, 64, 63, 22, 13, 7, 4, 3, 2, 1]
SOFTMAX_LENS = [1, 63, 64, 65, 70]


def _stats_inputs(cpg, groups=32, T=70):
    """x [B][cpg * groups][T] and its copy with NaN behind every row's end (nothing there is read)"""
    B, Cn = len(STATS_LENS), cpg * groups
    x = torch.from_numpy(synth.prng.normal(83 + cpg, B * Cn * T).reshape(B, Cn, T).copy()).float()
    xp = x.clone()
    for b, n in enumerate(STATS_LENS):
        xp[b, :, n:] = float("nan")
    return x, xp


def _softmax_inputs(T=70):
    """scores [B][T][T] and their copy with NaN outside every row's own block"""
    B = len(SOFTMAX_LENS)
    s = torch.from_numpy(synth.prng.normal(89, B * T * T).reshape(B, T, T).copy()).float() * 4.0
    sp = s.clone()
    for b, n in enumerate(SOFTMAX_LENS):
        sp[b, n:, :] = float("nan")
        sp[b, :, n:] = float("nan")
    return s, sp


@pytest.mark.parametrize("cpg", [1, 2, 4, 12])
def test_gn_stats_lens_unit_equals_the_plain_kernel_on_the_compacted_clip(ctx, cpg):
    lib, groups, T = ctx.lib, 32, 70
    Cn = cpg * groups
    lens = STATS_LENS
    B = len(lens)
    x, xp = _stats_inputs(cpg)
    xd = xp.cuda()
    mean = torch.full((B, groups), float("nan"), device="cuda")
    rstd = torch.full((B, groups), float("nan"), device="cuda")
    assert lib.vb_gn_stats_lens(L.ptr(xd), B, Cn, T, groups, L.ptr(_dev_lens(lens)), L.ptr(mean), L.ptr(rstd), L.stream_ptr()) == 0, lib.vb_last_error()
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        clip = x[b:b + 1, :, :n].contiguous().cuda()
        m1 = torch.empty(1, groups, device="cuda")
        r1 = torch.empty(1, groups, device="cuda")
        assert lib.vb_gn_stats_lens(L.ptr(clip), 1, Cn, n, groups, None, L.ptr(m1), L.ptr(r1), L.stream_ptr()) == 0, lib.vb_last_error()
        torch.cuda.synchronize()
        assert torch.equal(mean[b:b + 1], m1) and torch.equal(rstd[b:b + 1], r1), f"cpg {cpg}, row {b} (length {n}): not the plain kernel's bits"
        g64 = x[b, :, :n].double().reshape(groups, cpg * n)
        mu, var = g64.mean(1), g64.var(1, unbiased=False)
        # fp32 sums of at most 840 terms of unit scale: 1e-5 absolute on the mean, 1e-4 relative on rstd (eps = 1e-6 keeps one-sample groups finite)
        assert float((mean[b].cpu().double() - mu).abs().max()) < 1e-5
        ref = (var + 1e-6).rsqrt()
        assert float(((rstd[b].cpu().double() - ref).abs() / ref).max()) < 1e-4


def test_softmax_rows_t_lens_unit_equals_the_plain_kernel_on_the_compacted_scores(ctx):
    lib, T = ctx.lib, 70
    lens = SOFTMAX_LENS
    B = len(lens)
    s, sp = _softmax_inputs()
    out = torch.full((B, T, T), float("nan"), device="cuda")
    sd = sp.cuda()
    assert lib.vb_softmax_rows_t_lens(L.ptr(sd), B, T, L.ptr(_dev_lens(lens)), L.ptr(out), L.stream_ptr()) == 0, lib.vb_last_error()
    torch.cuda.synchronize()
    out = out.cpu()
    for b, n in enumerate(lens):
        blk = s[b:b + 1, :n, :n].contiguous().cuda()
        o1 = torch.empty(1, n, n, device="cuda")
        assert lib.vb_softmax_rows_t_lens(L.ptr(blk), 1, n, None, L.ptr(o1), L.stream_ptr()) == 0, lib.vb_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out[b, :n, :n], o1[0].cpu()), f"row {b} (length {n}): not the plain kernel's bits"
        ref = torch.softmax(s[b, :n, :n].double(), dim=-1).t()
        assert float((out[b, :n, :n].double() - ref).abs().max()) < 1e-6          # (probabilities <= 1: a few fp32 ulps of expf and the sum)
        assert int(torch.count_nonzero(out[b, n:, :])) == 0 and int(torch.count_nonzero(out[b, :, n:])) == 0
    assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_no_lengths_a_null_table_and_all_full_lengths_are_the_plain_call(nets, cfg, prec):
    net, B, T = nets[(cfg, prec)], 3, 24
    z = z_batch(T, B)
    plain = net.run(z).cpu()
    assert torch.equal(net.decode_lens(z, [T] * B).cpu(), plain) and torch.equal(net.decode_lens(z, None).cpu(), plain)
    lib = net.ctx.lib
    assert lib.vb_vae_decode_lens_workspace_bytes(net.ctx.handle, B, T) > lib.vb_net_workspace_bytes(net.ctx.handle, L.NET_VAE, B, T) + B * ZC * T * 4
    for lens in (None, L.Lens(None), L.Lens((C.c_int32 * B)(*[T] * B))):
        rc, msg, out = c_call(net, z, lens)
        assert rc == 0, msg
        assert torch.equal(out, plain)


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals_name_the_row_or_the_limit_and_leave_mel_untouched(nets):
    net, T = nets[("narrow", "fp32mf")], 24

    def call(lens):
        rc, msg, mel = c_call(net, torch.zeros(len(lens), ZC, T), L.Lens((C.c_int32 * len(lens))(*lens)), out_fill=7.0)
        assert bool((mel == 7.0).all()), "a refused call must not touch mel"
        return rc, msg

    rc, msg = call([24, 0, 12])
    assert rc == -1 and b"row 1" in msg and b"length 0" in msg
    rc, msg = call([24, 12, 25])
    assert rc == -1 and b"row 2" in msg and b"length 25" in msg
    rc, msg = call([12] * 65)
    assert rc == -1 and b"65 rows" in msg and b"1..64" in msg
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0"), ([24, 12, 25], r"lengths\[2\] = 25"), ([12] * 65, "65 rows")):
        with pytest.raises(ValueError, match=text):
            net.decode_lens(torch.zeros(len(lens), ZC, T), lens)


def test_decode_lens_on_the_encoder_and_on_a_vocoder_raises_naming_the_net(ctx):
    from versband_amd.engine import build_hifigan, build_vae_encoder
    enc = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(CONFIGS["narrow"]), SEED + 3), precision="fp32")
    with pytest.raises(ValueError, match="VAE encoder"):
        enc.decode_lens(torch.zeros(2, enc.in_ch, 16 * enc.in_tmul), [16, 8])
    hcfg = synth.HifiGanConfig(upsample_initial_channel=256)
    voc = build_hifigan(ctx, synth.make_state_dict(synth.hifigan_shapes(hcfg), SEED + 2), hcfg.as_hparams(), precision="fp32")
    with pytest.raises(ValueError, match="vocoder"):
        voc.decode_lens(torch.zeros(2, 80, 16), [16, 8])


def test_model_decode_first_stage_takes_lengths(nets):
    from versband_amd import model as vm
    net = nets[("narrow", "split")]
    stub = type("M", (), {"vae_net": lambda self: net})()
    T, lens = SAME_ROUTE["one"]
    mel = vm.CFM.decode_first_stage(stub, padded(T, lens), lengths=lens).cpu()
    assert torch.equal(mel, lens_run(nets, "narrow", "split", T, lens))
    assert torch.equal(vm.CFM.decode_first_stage(stub, z_batch(T, 2)).cpu(), net.run(z_batch(T, 2)).cpu())


# ---------------------------------------------------------------------------------------------------------------- 9
def test_cli_decode_lengths_files_are_byte_identical(tmp_path):
    """scripts/infer_batched.py --items_per_batch 6 --length_slack 8 over items of 150, 152, 151, 153, 150, 154 latent tokens: by the
    route rule 150, 150 and 154 share one decode call with row lengths, so the group decodes in four calls for five distinct lengths -
    against --length_slack 0: the same files byte for byte"""
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
    dec = harness.plan_decode_calls(tokens)
    assert len(dec) < len(set(tokens)) and any(c["lengths"] for c in dec)
    assert [c["rows"] for c in dec] == [[0, 4, 5], [1], [2], [3]] and dec[0]["lengths"] == [150, 150, 154]


# --------------------------------------------------------------------------------------------------------------- 10
def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# sha256 of the raw output bytes as commit e576ae7 produced them on an MI355X - the last commit with a statistics kernel and a transposed
# softmax per form, before the two forms became instantiations of one body (at T = 5 the narrow program runs the same kernels in fp32 and
# fp32mf, and in bf16 and bf16xt: the equal digests).  "lens": the call with the length table (statistics: mean then
# rstd [B][groups]; softmax: the whole [B][T][T]); "plain": the calls with len = NULL on the compacted clips, row after row (statistics:
# mean then rstd of each; softmax: each [n][n] block).  "decode": ConvNet.decode_lens of the narrow program on SAME_ROUTE["one"].
PARENT_BITS = {
    "gn_stats cpg 1 lens": "cb7e59582088b752c3e64b04e4117b6f5123c493d7ab596b54eed45027236cb9",
    "gn_stats cpg 1 plain": "3a5dbe147b98263c5b684cdf1f6bee2cc9a64ddbf3c5d72739f26242fcd9448b",
    "gn_stats cpg 2 lens": "140295b662f09e50967575f5ce944cc54036a53bbfb539dae4e7189045f0f4eb",
    "gn_stats cpg 2 plain": "700e5a1f06de96e7c4d528239709d7bf2c6a8ca7c7352ed13b0b45c17461b226",
    "gn_stats cpg 4 lens": "e31ca822c3ae9ca711c760d81aa8eec659209c61e151f7b846a795d101486143",
    "gn_stats cpg 4 plain": "327f2de717bf9338449bc17bff92ccdce681c69550139fcd74f7507a9936e24b",
    "gn_stats cpg 12 lens": "646364e3dd9caf01ec0bf8317b1df3f1e5f0e8c4c5bf1e59af87820ba8be8e06",
    "gn_stats cpg 12 plain": "47243e63c476e6e9e717a4afbf4196e7477f0ef4142354d9dbf9f07385848870",
    "softmax_rows_t lens": "cf5edc442e8e60979aa838da409d046aa2ca6800352a773b0e62b87e94b350c7",
    "softmax_rows_t plain": "8394c62ac345f658fe348b6ce0425c32a9d0af3be58745f6e4d1ce25be68230c",
    "decode narrow fp32": "deb444bd8b20ae9aa6219d78adb426864b5fce475f544e1aaf815631e15b278b",
    "decode narrow fp32mf": "deb444bd8b20ae9aa6219d78adb426864b5fce475f544e1aaf815631e15b278b",
    "decode narrow split": "f67de97be3243582d4672873799a7a5658f5e450295588dc2181aa9d6475ef0b",
    "decode narrow bf16": "5c45a578ac80a56a01d7afa339ec6fd6cd062255679bcb6855954a0dd14711b1",
    "decode narrow bf16xt": "5c45a578ac80a56a01d7afa339ec6fd6cd062255679bcb6855954a0dd14711b1",
}


def test_glue_kernels_keep_the_bits_of_the_two_kernel_pairs_they_replace(ctx):
    lib, groups, T = ctx.lib, 32, 70
    got = {}
    for cpg in (1, 2, 4, 12):
        Cn, B = cpg * groups, len(STATS_LENS)
        x, xp = _stats_inputs(cpg)
        mean = torch.full((B, groups), float("nan"), device="cuda")
        rstd = torch.full((B, groups), float("nan"), device="cuda")
        assert lib.vb_gn_stats_lens(L.ptr(xp.cuda()), B, Cn, T, groups, L.ptr(_dev_lens(STATS_LENS)), L.ptr(mean), L.ptr(rstd), L.stream_ptr()) == 0, lib.vb_last_error()
        torch.cuda.synchronize()
        got[f"gn_stats cpg {cpg} lens"] = _sha(mean, rstd)
        rows = []
        for b, n in enumerate(STATS_LENS):
            clip = x[b:b + 1, :, :n].contiguous().cuda()
            m1 = torch.full((1, groups), float("nan"), device="cuda")
            r1 = torch.full((1, groups), float("nan"), device="cuda")
            assert lib.vb_gn_stats_lens(L.ptr(clip), 1, Cn, n, groups, None, L.ptr(m1), L.ptr(r1), L.stream_ptr()) == 0, lib.vb_last_error()
            torch.cuda.synchronize()
            rows += [m1, r1]
        got[f"gn_stats cpg {cpg} plain"] = _sha(*rows)
    s, sp = _softmax_inputs()
    B = len(SOFTMAX_LENS)
    out = torch.full((B, T, T), float("nan"), device="cuda")
    assert lib.vb_softmax_rows_t_lens(L.ptr(sp.cuda()), B, T, L.ptr(_dev_lens(SOFTMAX_LENS)), L.ptr(out), L.stream_ptr()) == 0, lib.vb_last_error()
    torch.cuda.synchronize()
    got["softmax_rows_t lens"] = _sha(out)
    rows = []
    for b, n in enumerate(SOFTMAX_LENS):
        blk = s[b:b + 1, :n, :n].contiguous().cuda()
        o1 = torch.full((1, n, n), float("nan"), device="cuda")
        assert lib.vb_softmax_rows_t_lens(L.ptr(blk), 1, n, None, L.ptr(o1), L.stream_ptr()) == 0, lib.vb_last_error()
        torch.cuda.synchronize()
        rows.append(o1)
    got["softmax_rows_t plain"] = _sha(*rows)
    assert sorted(got) == sorted(k for k in PARENT_BITS if not k.startswith("decode"))
    for name, digest in got.items():
        assert digest == PARENT_BITS.get(name), f"{name}: sha256 {digest}, not the parent's {PARENT_BITS.get(name)}"


@pytest.mark.parametrize("prec", PRECISIONS)
def test_narrow_lens_decode_keeps_the_parent_bits(nets, prec):
    T, lens = SAME_ROUTE["one"]
    assert T == min(t for t, _ in SAME_ROUTE.values()) and T < MIXED[0]
    digest = _sha(lens_run(nets, "narrow", prec, T, lens))
    assert digest == PARENT_BITS.get(f"decode narrow {prec}"), f"decode narrow {prec}: sha256 {digest}, not the parent's {PARENT_BITS.get(f'decode narrow {prec}')}"
