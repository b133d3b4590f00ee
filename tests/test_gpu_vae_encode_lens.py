"""VAE encoder with row lengths on the GPU (vb_vae_encode_lens, ConvNet.encode_lens, encode_first_stage(lengths=)) and the posterior
with row lengths (vb_posterior_lens): mels of different lengths as rows of one encode call.  The contract of include/versband_hip.h: T and
the lengths count LATENT tokens, row b owns in_tmul * len[b] mel frames, its first len[b] columns of the moments are vb_vae_encode on that
clip alone - bit for bit when len[b] and the padded T agree by the route rule (harness.ENCODE_ROUTE_MOD), to the precision's roundoff
otherwise - the rest of the row is exact zeros, and neither the caller's mel padding nor anything in the workspace is read.

"narrow" = VAEConfig(ch=32) in all five precisions (GroupNorm inside the register-staged convolutions, scalar statistics at odd lengths),
"wide" = VAEConfig() in fp32mf, split and bf16xt (gn_apply, xt_planes and the DMA-fed GEMM).  Both hold one Downsample1D: the pair of
in_stride = 2 convolutions whose last output of a row reaches for the first sample behind the row's end.  A one-token row is two mel frames
and its only down-convolution output reads x[2], the first tail sample: the smallest shape at which the right pad can go wrong.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, describe, rel_l2
from versband_amd import _lib as L
from versband_amd import harness, pack, synth

pytestmark = pytest.mark.gpu
VB_E_INVALID = -1
CONFIGS = {"narrow": synth.VAEConfig(ch=32), "wide": synth.VAEConfig()}
PRECISIONS = {"narrow": ("fp32", "fp32mf", "split", "bf16", "bf16xt"), "wide": ("fp32mf", "split", "bf16xt")}
NETS = [(c, p) for c in CONFIGS for p in PRECISIONS[c]]
M = harness.ENCODE_ROUTE_MOD
SAME_ROUTE = {"r0": (96, [96, 68, 36, 4]), "r2": (70, [70, 66, 38, 6, 2]), "one": (5, [5, 1])}
MIXED = (24, [24, 22, 13, 7, 1])          # every residue mod 4, odd lengths, a one-token row
MELS, E = 80, 20


@functools.lru_cache(maxsize=None)
def state(cfg_name):
    sd = synth.make_state_dict(synth.vae_encoder_shapes(CONFIGS[cfg_name]), SEED + 3)
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def mel_batch(T, B):
    """B mels of 2 T frames (T latent tokens); never modified (callers clone before they write padding)"""
    return torch.from_numpy(synth.prng.normal(97, B * MELS * 2 * T).reshape(B, MELS, 2 * T).copy()).float()


def padded(T, lens, fill=0.0):
    x = mel_batch(T, len(lens)).clone()
    for b, n in enumerate(lens):
        x[b, :, 2 * n:] = fill
    return x


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from versband_amd.engine import Context
    return Context("cuda:0")


@pytest.fixture(scope="module")
def nets(ctx):
    from versband_amd.engine import build_vae_encoder
    return {(c, p): build_vae_encoder(ctx, state(c)[0], precision=p) for c, p in NETS}


_cache = {}


def lens_run(nets, cfg, prec, T, lens):
    """the zero-padded call with lengths, once per (program, precision, batch): the reference of checks 1 to 4"""
    key = (cfg, prec, T, tuple(lens))
    if key not in _cache:
        _cache[key] = nets[(cfg, prec)].encode_lens(padded(T, lens), lens).cpu()
    return _cache[key]


def alone(nets, cfg, prec, T, B, b, n):
    """the plain call on row b's clip alone"""
    key = ("alone", cfg, prec, T, B, b, n)
    if key not in _cache:
        _cache[key] = nets[(cfg, prec)].run(mel_batch(T, B)[b:b + 1, :, :2 * n].contiguous()).cpu()
    return _cache[key]


def test_the_sets_follow_the_documented_rule_and_the_programs_hold_the_strided_pair(nets):
    assert M == 4
    for T, lens in SAME_ROUTE.values():
        assert all(n % M == T % M for n in lens) and lens[0] == T
        assert [c["rows"] for c in harness.plan_encode_calls(lens)] == [list(range(len(lens)))]
    assert {n % 4 for n in MIXED[1]} == {0, 1, 2, 3} and 1 in MIXED[1] and 1 in SAME_ROUTE["one"][1]
    for (cfg, prec), net in nets.items():
        assert net.in_tmul == 2 and net.out_tmul == 1 and net.out_ch == 2 * E
        pair = [op for op in net.nb.ops if op.kind == L.OP_CONV and op.in_stride == 2]
        assert [(op.in_phase, op.in_act, op.stats, op.beta) for op in pair] == [(0, L.ACT_NONE, -1, 0.0), (1, L.ACT_NONE, -1, 1.0)], (cfg, prec)
        assert any(op.kind == L.OP_SOFTMAX_T for op in net.nb.ops) and any(op.kind == L.OP_GN_STATS for op in net.nb.ops)
    kinds = {(c, op.kind) for (c, _), net in nets.items() for op in net.nb.ops}
    assert ("wide", L.OP_GN_APPLY) in kinds and ("wide", L.OP_XT_PLANES) in kinds
    assert any(op.kind == L.OP_CONV and op.stats >= 0 for op in nets[("narrow", "split")].nb.ops)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(SAME_ROUTE))
@pytest.mark.parametrize("cfg,prec", NETS)
def test_rows_equal_the_clip_alone_bit_for_bit(nets, cfg, prec, name):
    T, lens = SAME_ROUTE[name]
    mom = lens_run(nets, cfg, prec, T, lens)
    assert mom.shape == (len(lens), 2 * E, T)
    for b, n in enumerate(lens):
        ref = alone(nets, cfg, prec, T, len(lens), b, n)
        got = mom[b:b + 1, :, :n]
        assert torch.equal(got, ref), describe(f"{cfg} {prec} {name}: row {b} (length {n} of {T}) vs the clip alone", got, ref)
        assert int(torch.count_nonzero(mom[b, :, n:])) == 0, f"{cfg} {prec} {name}: row {b} has nonzero moments behind its end"
        assert torch.isfinite(mom[b]).all() and float(got.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("name", list(SAME_ROUTE))
@pytest.mark.parametrize("cfg,prec", NETS)
def test_padding_is_never_read(nets, cfg, prec, name, fill):
    T, lens = SAME_ROUTE[name]
    mom = nets[(cfg, prec)].encode_lens(padded(T, lens, fill), lens).cpu()
    assert torch.isfinite(mom).all(), f"{cfg} {prec} {name}: padding of {fill} reached the output"
    assert torch.equal(mom, lens_run(nets, cfg, prec, T, lens)), f"{cfg} {prec} {name}: the result depends on the mel padding"


# ---------------------------------------------------------------------------------------------------------------- 3
def c_call(net, x, T, lens, ws_fill=None, out_fill=float("nan"), out_shape=None):
    """vb_vae_encode_lens through the C ABI with a caller-owned workspace; returns (rc, message, moments on the host)"""
    lib = net.ctx.lib
    B = x.shape[0]
    x = x.cuda().contiguous()
    ws = torch.empty(max(256, lib.vb_vae_encode_lens_workspace_bytes(net.ctx.handle, B, T)), dtype=torch.uint8, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    out = torch.full(out_shape or (B, net.out_ch, T * net.out_tmul), out_fill, device="cuda")
    rc = lib.vb_vae_encode_lens(net.ctx.handle, L.ptr(x), B, T, C.byref(lens) if lens is not None else None, L.ptr(out), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, lib.vb_last_error(), out.cpu()


def _lens(vals):
    return L.Lens((C.c_int32 * len(vals))(*vals))


@pytest.mark.parametrize("name", ["r2", "one"])
@pytest.mark.parametrize("cfg,prec", NETS)
def test_the_workspace_is_never_read(nets, cfg, prec, name):
    T, lens = SAME_ROUTE[name]
    net = nets[(cfg, prec)]
    outs = []
    for fill in (0xFF, 0x00):
        rc, msg, mom = c_call(net, padded(T, lens), T, _lens(lens), ws_fill=fill)
        assert rc == 0, msg
        assert torch.isfinite(mom).all(), f"{cfg} {prec} {name}: a workspace of {fill:#x} bytes reached the output"
        outs.append(mom)
    assert torch.equal(outs[0], outs[1]), describe(f"{cfg} {prec} {name}: 0xFF workspace vs zeroed", outs[0], outs[1])
    assert torch.equal(outs[0], lens_run(nets, cfg, prec, T, lens))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("cfg,prec", NETS)
def test_rows_are_independent_of_their_neighbours(nets, cfg, prec):
    T, lens = SAME_ROUTE["r2"]
    base = lens_run(nets, cfg, prec, T, lens)
    x = padded(T, lens)
    other = list(lens)
    x[0] = mel_batch(T, len(lens) + 1)[len(lens)]                # another clip in row 0 ...
    other[0], other[2] = 33, 70                                   # ... of another length (and residue); row 2 grows to the full T
    x[0, :, 2 * 33:] = 0.0
    x[2] = mel_batch(T, len(lens))[2]
    mom = nets[(cfg, prec)].encode_lens(x, other).cpu()
    for b in (1, 3, 4):
        assert torch.equal(mom[b], base[b]), describe(f"{cfg} {prec}: row {b} changed with its neighbours", mom[b], base[b])
    assert torch.equal(mom[2:3], alone(nets, cfg, prec, T, len(lens), 2, T))          # (row 2 is the full clip now)


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("cfg,prec", NETS)
def test_no_lengths_a_null_table_and_all_full_lengths_are_the_plain_call(nets, cfg, prec):
    net, B, T = nets[(cfg, prec)], 3, 24
    x = mel_batch(T, B)
    plain = net.run(x).cpu()
    assert torch.equal(net.encode_lens(x, [T] * B).cpu(), plain) and torch.equal(net.encode_lens(x, None).cpu(), plain)
    lib = net.ctx.lib
    assert lib.vb_vae_encode_lens_workspace_bytes(net.ctx.handle, B, T) >= (lib.vb_net_workspace_bytes(net.ctx.handle, L.NET_VAE_ENCODER, B, T)
                                                                            + B * MELS * 2 * T * 4 + 64 * 4)
    for lens in (None, L.Lens(None), _lens([T] * B)):
        rc, msg, out = c_call(net, x, T, lens)
        assert rc == 0, msg
        assert torch.equal(out, plain)


# ---------------------------------------------------------------------------------------------------------------- 6
@functools.lru_cache(maxsize=None)
def oracle_row(cfg, b):
    """float64 oracle of row b of MIXED on the clip alone; computed once, never modified.  The clip goes in twice and row 0 is kept:
    torch's group_norm refuses a batch of one whose groups hold one value (the one-token clip of the 32-channel program: cpg = 1, one
    sample at the latent rate), a guard for training that changes no value - batch rows are normalised one by one."""
    T, lens = MIXED
    x = mel_batch(T, len(lens))[b:b + 1, :, :2 * lens[b]].contiguous()
    return ref_cpu.vae_encode(state(cfg)[1], torch.cat([x, x]).double())[:1].contiguous()


@pytest.mark.parametrize("cfg,prec", NETS)
def test_mixed_residues_stay_within_twice_the_clip_alones_error(nets, cfg, prec):
    """Per precision e_alone = rel-L2 of the plain call on the clip alone against the float64 oracle; a row of the lengths call may run the
    direct kernel where the clip alone runs minimal filtering (or the other way round), both inside the precision's class: the row is held
    to 2 * max(e_alone, 1e-6).  Rows of T's residue stay bit-equal."""
    T, lens = MIXED
    mom = nets[(cfg, prec)].encode_lens(padded(T, lens), lens).cpu()
    for b, n in enumerate(lens):
        orc = oracle_row(cfg, b)
        assert orc.shape == (1, 2 * E, n)
        ref = alone(nets, cfg, prec, T, len(lens), b, n)
        e_alone, e_row = rel_l2(ref, orc), rel_l2(mom[b:b + 1, :, :n], orc)
        print(f"[{cfg} {prec}] row {b} (length {n} of {T}): e_alone {e_alone:.3e}, e_row {e_row:.3e}")
        assert e_row <= 2 * max(e_alone, 1e-6), describe(f"{cfg} {prec} row {b} vs float64", mom[b:b + 1, :, :n], orc)
        assert int(torch.count_nonzero(mom[b, :, n:])) == 0
        if n % M == T % M:
            assert torch.equal(mom[b:b + 1, :, :n], ref), f"{cfg} {prec}: row {b} shares T's residue and is not the clip alone's bits"


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_name_the_row_or_the_op_and_leave_the_moments_untouched(ctx, nets):
    from versband_amd.engine import ConvNet, NetBuilder, build_vae_decoder
    net, T = nets[("narrow", "fp32mf")], 24

    def call(n, x, T, lens, shape=None):
        rc, msg, out = c_call(n, x, T, _lens(lens), out_fill=7.0, out_shape=shape)
        assert bool((out == 7.0).all()), "a refused call must not touch the moments"
        return rc, msg

    rc, msg = call(net, torch.zeros(3, MELS, 2 * T), T, [24, 0, 12])
    assert rc == VB_E_INVALID and b"row 1" in msg and b"length 0" in msg
    rc, msg = call(net, torch.zeros(3, MELS, 2 * T), T, [24, 12, 25])
    assert rc == VB_E_INVALID and b"row 2" in msg and b"length 25" in msg
    rc, msg = call(net, torch.zeros(65, MELS, 2 * T), T, [12] * 65)
    assert rc == VB_E_INVALID and b"65 rows" in msg and b"1..64" in msg
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0"), ([24, 12, 25], r"lengths\[2\] = 25"), ([12] * 65, "65 rows")):
        with pytest.raises(ValueError, match=text):
            net.encode_lens(torch.zeros(len(lens), MELS, 2 * T), lens)
    # the decoder's program in the encoder's slot: it upsamples
    dec = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(CONFIGS["narrow"]), SEED + 1), precision="fp32")
    assert any(op.upsample2 for op in dec.nb.ops)
    as_enc = ConvNet(ctx, L.NET_VAE_ENCODER, dec.nb, dec.in_ch, dec.out_ch, dec.out_tmul, in_tmul=1)
    rc, msg = call(as_enc, torch.zeros(2, dec.in_ch, T), T, [24, 12])
    assert rc == VB_E_INVALID and b"vae_encode_lens: op " in msg and b"upsample2" in msg and b"not an op of the VAE encoder's program" in msg, msg
    # a down-convolution that activates its input pads the ACTIVATED row: a hand-made two-op program
    nb = NetBuilder(ctx.device, "fp32")
    w = torch.from_numpy(synth.prng.normal(5, 8 * 8 * 2).reshape(8, 8, 2).copy()).float()
    h = nb.buf(8, 1)
    nb.conv(L.BUF_INPUT, h, 8, 8, pack.pack_conv(w), torch.zeros(8), k=2, in_stride=2, in_phase=0, in_act=L.ACT_LRELU, in_slope=0.1)
    nb.conv(h, L.BUF_OUTPUT, 8, 8, pack.pack_conv(w[:, :, :1].contiguous()), torch.zeros(8))
    two = ConvNet(ctx, L.NET_VAE_ENCODER, nb, 8, 8, 1, in_tmul=2)
    rc, msg = call(two, torch.zeros(2, 8, 2 * T), T, [24, 12])
    assert rc == VB_E_INVALID and b"vae_encode_lens: op 0 (VB_OP_CONV)" in msg and b"in_stride = 2" in msg and b"activation" in msg, msg
    # and the decoder's own entry point goes on refusing the encoder's strided pair
    lib = net.ctx.lib
    enc_as_dec = ConvNet(ctx, L.NET_VAE, net.nb, net.in_ch, net.out_ch, 1, in_tmul=1)
    ws = torch.empty(max(256, lib.vb_vae_decode_lens_workspace_bytes(enc_as_dec.ctx.handle, 2, T)), dtype=torch.uint8, device="cuda")
    out = torch.full((2, net.out_ch, T), 7.0, device="cuda")
    x = torch.zeros(2, MELS, T, device="cuda")
    rc = lib.vb_vae_decode_lens(enc_as_dec.ctx.handle, L.ptr(x), 2, T, C.byref(_lens([24, 12])), L.ptr(out), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == VB_E_INVALID and b"in_stride" in lib.vb_last_error() and bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 8
def _posterior_inputs(T, lens):
    B = len(lens)
    mom = torch.from_numpy(synth.prng.normal(101 + T, B * 2 * E * T).reshape(B, 2 * E, T).copy()).float()
    mom[:, E, 0], mom[:, E + 1, 0] = -40.0, 30.0                 # both clamps of logvar, in every row's first (valid) column
    eps = torch.from_numpy(synth.prng.normal(103 + T, B * E * T).reshape(B, E, T).copy()).float()
    mom_p, eps_p = mom.clone(), eps.clone()
    for b, n in enumerate(lens):
        mom_p[b, :, n:] = float("nan")
        eps_p[b, :, n:] = float("nan")
    return mom, eps, mom_p, eps_p


def _posterior(lib, mom, eps, lens, scale):
    B, T = mom.shape[0], mom.shape[2]
    z = torch.full((B, E, T), float("nan"), device="cuda")
    md, ed = mom.cuda(), (eps.cuda() if eps is not None else None)
    arr = (C.c_int32 * B)(*lens) if lens is not None else None
    rc = lib.vb_posterior_lens(L.ptr(md), L.ptr(ed), B, E, T, arr, scale, L.ptr(z), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.vb_last_error()
    return z.cpu()


@pytest.mark.parametrize("T,lens", [(24, [24, 13, 1]), (7, [7, 2])])
def test_posterior_lens_mode_sample_and_tails(ctx, T, lens):
    lib, scale = ctx.lib, 0.37
    s32 = torch.tensor(scale, dtype=torch.float32)
    mom, eps, mom_p, eps_p = _posterior_inputs(T, lens)
    # the mode: float32(scale) * mean bit for bit, exact zeros behind each row's end although moments (and noise) are NaN there
    z = _posterior(lib, mom_p, None, lens, scale)
    zs = _posterior(lib, mom_p, eps_p, lens, scale)
    mean64, lv64 = mom[:, :E].double(), mom[:, E:].double().clamp(-30.0, 20.0)
    std_eps = torch.exp(0.5 * lv64) * eps.double()
    z64 = float(s32) * (mean64 + std_eps)
    bound = 8 * 2.0 ** -24 * abs(float(s32)) * (mean64.abs() + std_eps.abs())
    assert float(lv64.min()) == -30.0 and float(lv64.max()) == 20.0
    for b, n in enumerate(lens):
        assert torch.equal(z[b, :, :n], s32 * mom[b, :E, :n]), f"mode, row {b}"
        for name, t in (("mode", z), ("sample", zs)):
            assert int(torch.count_nonzero(t[b, :, n:])) == 0 and torch.isfinite(t[b]).all(), f"{name}: row {b} is not zero behind its end"
        err = (zs[b, :, :n].double() - z64[b, :, :n]).abs()
        print(f"[posterior T={T}] row {b}: max err / bound {float((err / bound[b, :, :n]).max()):.3f}")
        assert bool((err <= bound[b, :, :n]).all()), f"sample, row {b}: {float((err / bound[b, :, :n]).max()):.3f} x the bound"
    # len = NULL: full rows, the same values where the rows are valid
    full = _posterior(lib, mom, eps, None, scale)
    for b, n in enumerate(lens):
        assert torch.equal(full[b, :, :n], zs[b, :, :n])
    assert bool(((full.double() - z64).abs() <= bound).all())
    # refusals: the row is named, z untouched
    zt = torch.full((len(lens), E, T), 7.0, device="cuda")
    bad = (C.c_int32 * len(lens))(*([T + 1] + list(lens[1:])))
    rc = lib.vb_posterior_lens(L.ptr(mom.cuda()), None, len(lens), E, T, bad, scale, L.ptr(zt), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == VB_E_INVALID and b"row 0" in lib.vb_last_error() and bool((zt == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 9
def test_model_encodes_samples_and_decodes_with_lengths(ctx, nets):
    from versband_amd import model as vm
    from versband_amd.engine import build_vae_decoder
    enc = nets[("narrow", "split")]
    scale = 0.41
    dec = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(CONFIGS["narrow"]), SEED + 1), scale_factor=scale, precision="split")
    fs = object.__new__(vm.AutoencoderKL)
    fs.enc_net, fs.enc_state = enc, {"loaded": True}

    class Model:
        first_stage_model, scale_factor = fs, torch.tensor(scale)
        encode_first_stage, get_first_stage_encoding = vm.CFM.encode_first_stage, vm.CFM.get_first_stage_encoding
        _posterior_lens, decode_first_stage = vm.CFM._posterior_lens, vm.CFM.decode_first_stage

        def _context(self):
            return ctx

        def vae_net(self):
            return dec

    m = Model()
    T, lens = SAME_ROUTE["one"]
    x = padded(T, lens, float("nan"))
    post = m.encode_first_stage(x, lengths=lens)
    assert isinstance(post, vm.DiagonalGaussianDistribution)
    assert torch.equal(post.parameters.cpu(), lens_run(nets, "narrow", "split", T, lens))
    z = m.get_first_stage_encoding(post, lengths=lens, mode=True)
    assert torch.equal(z.cpu(), torch.tensor(scale, dtype=torch.float32) * lens_run(nets, "narrow", "split", T, lens)[:, :E])
    zs = m.get_first_stage_encoding(post, lengths=lens).cpu()
    assert zs.shape == (len(lens), E, T) and torch.isfinite(zs).all()
    for b, n in enumerate(lens):
        assert int(torch.count_nonzero(zs[b, :, n:])) == 0 and float(zs[b, :, :n].abs().max()) > 0
    # without lengths: the path before this feature - enc.run, DiagonalGaussianDistribution.sample, the scale in torch
    full = mel_batch(T, 2)
    assert torch.equal(m.encode_first_stage(full).parameters.cpu(), enc.run(full).cpu())
    eps = torch.from_numpy(synth.prng.normal(107, 2 * E * T).reshape(2, E, T).copy()).float()
    plain = m.encode_first_stage(full)
    assert torch.equal(m.get_first_stage_encoding(plain.mode()).cpu(), (scale * plain.mean).cpu())
    # (full rows with a given draw: the kernel against the elementwise path, each within the posterior test's bound of the exact value)
    both = 2 * 8 * 2.0 ** -24 * scale * (plain.mean.abs() + (plain.std * eps.to(plain.std.device)).abs()).cpu().double()
    diff = (m.get_first_stage_encoding(plain, lengths=[T, T], noise=eps).cpu().double() - (scale * plain.sample(eps)).cpu().double()).abs()
    assert bool((diff <= both).all())
    # round trip: the encoded latents, decoded with the same lengths
    mel = m.decode_first_stage(z, lengths=lens).cpu()
    assert mel.shape == (len(lens), MELS, 2 * T) and torch.isfinite(mel).all()
    for b, n in enumerate(lens):
        assert int(torch.count_nonzero(mel[b, :, 2 * n:])) == 0 and float(mel[b, :, :2 * n].abs().max()) > 0
