"""BigVGAN with row lengths on the GPU (vb_bigvgan_forward_lens / vb_bigvgan_forward_chunked_lens, ConvNet.vocode_lens,
VocoderBigVGAN.vocode_batch, and the unit vb_aa_act): mels of different lengths as rows of one vocoder call.  The contract of
include/versband_hip.h: row b's first len[b] * hop samples are the call on that clip alone - bit for bit when len[b] and the padded T agree
mod 4, to the precision's roundoff otherwise - the rest of the row is exact zeros, and the caller's mel padding is never read.

What stood in the way was one kernel: the anti-aliased activation replicate-pads at the row end (tests/test_bigvgan_lens_host.py measures
how far a zero tail reaches into a row).  With a length table it takes the row's own end for its three bounds and writes the zeros behind it.

Two programs, so both AMP block forms and both activations run:
  amp1  synth.BigVGANConfig(upsample_initial_channel=256): AMPBlock1, SnakeBeta, log-scale; 128 / 64 / 32 / 16 channels at 8 / 40 / 160 / 320
        samples per frame, in the five precisions
  amp2  the amp2 configuration of tests/test_oracle_golden.py: AMPBlock2, Snake; in fp32 and bf16xt
The shapes are those of tests/test_gpu_vocoder_lens.py.  At 320 samples per frame against the activation's 256-output tile: length 4 ends on
a tile boundary (1280 = 5 x 256), length 22 inside a tile (7040), and at every stage short rows leave whole workgroups behind their end.
"""
import ctypes as C
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as TF

from oracle import ref_cpu
from tests.helpers import SEED, describe, rel_l2
from tests.test_bf16_mode import bf16_mode
from tests.test_oracle_golden import _BV_CFGS
from versband_amd import _lib as L
from versband_amd import harness, pack, synth

pytestmark = pytest.mark.gpu
PRECISIONS = ("fp32", "fp32mf", "split", "bf16", "bf16xt")
CFGS = {"amp1": synth.BigVGANConfig(upsample_initial_channel=256), "amp2": synth.BigVGANConfig(**_BV_CFGS["amp2"])}
PROGRAMS = [("amp1", p) for p in PRECISIONS] + [("amp2", "fp32"), ("amp2", "bf16xt")]
HOP = 320
# (a) / (b): every length agrees with T mod 4 - rows are bit-equal to the clip alone.  "one": a one-frame row beside a full one (1 = 5 mod 4)
SAME_RESIDUE = {"mod0": (24, [24, 20, 16, 12, 8, 4]), "mod2": (22, [22, 18, 10, 6, 2]), "one": (5, [5, 1])}
MIXED = (24, [24, 22, 13, 7])          # (c): residues 0, 2, 1, 3 under T = 24
CHUNKED = (40, 16, 4, [40, 28, 12])    # (f): T, chunk, halo, lengths - all multiples of 4
U32 = 2.0 ** -24


def ids(v):
    return "-".join(v) if isinstance(v, tuple) else None


@functools.lru_cache(maxsize=None)
def state(tag):
    sd = synth.make_state_dict(synth.bigvgan_shapes(CFGS[tag]), SEED + 7)
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
    from versband_amd.engine import build_bigvgan
    built = {}
    for tag, prec in PROGRAMS:
        net = build_bigvgan(ctx, state(tag)[0], CFGS[tag].as_hparams(), precision=prec)
        assert net.out_tmul == HOP and net.which == L.NET_VOCODER
        built[(tag, prec)] = net
    return built


_cache = {}


def lens_run(nets, prog, T, lens):
    """the zero-padded call with lengths, once per (program, batch): the reference of (a) and (b)"""
    key = (prog, T, tuple(lens))
    if key not in _cache:
        _cache[key] = nets[prog].vocode_lens(padded(T, lens), lens).cpu()
    return _cache[key]


def alone(nets, prog, T, B, b, n):
    """the plain call on row b's clip alone"""
    return nets[prog].run(mel_batch(T, B)[b:b + 1, :, :n].contiguous()).cpu()


def test_programs_hold_both_block_forms_and_the_stage_widths(nets):
    for (tag, prec), net in nets.items():
        acts = [op for op in net.nb.ops if op.kind == L.OP_AA_ACT]
        widths = sorted({op.Ci for op in acts})
        assert widths == ([16, 32, 64, 128] if tag == "amp1" else [8, 16, 32]), (tag, prec, widths)
        assert not any(op.kind == L.OP_RESPAIR for op in net.nb.ops)


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("name", list(SAME_RESIDUE))
@pytest.mark.parametrize("prog", PROGRAMS, ids=ids)
def test_rows_equal_the_clip_alone_bit_for_bit(nets, prog, name):
    T, lens = SAME_RESIDUE[name]
    wav = lens_run(nets, prog, T, lens)
    assert wav.shape == (len(lens), 1, T * HOP)
    for b, n in enumerate(lens):
        ref = alone(nets, prog, T, len(lens), b, n)
        got = wav[b:b + 1, :, :n * HOP]
        assert torch.equal(got, ref), describe(f"{prog} {name}: row {b} (length {n} of {T}) vs the clip alone", got, ref)
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0, f"{prog} {name}: row {b} has nonzero samples behind its end"
        assert torch.isfinite(wav[b]).all() and float(got.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("name", list(SAME_RESIDUE))
@pytest.mark.parametrize("prog", PROGRAMS, ids=ids)
def test_padding_is_never_read(nets, prog, name, fill):
    T, lens = SAME_RESIDUE[name]
    wav = nets[prog].vocode_lens(padded(T, lens, fill), lens).cpu()
    assert torch.isfinite(wav).all(), f"{prog} {name}: padding of {fill} reached the output"
    assert torch.equal(wav, lens_run(nets, prog, T, lens)), f"{prog} {name}: the result depends on the mel padding"


# ---------------------------------------------------------------------------------------------------------------- c
class _FiltersInTheNetsDtype:
    """torch.nn.functional for the float64 oracle: ref_cpu builds BigVGAN's anti-aliasing filters in fp32 whatever the net's dtype (the
    values the kernel multiplies by), so the depthwise filters are cast to the input's dtype; nothing else changes"""

    def __getattr__(self, name):
        return getattr(TF, name)

    def conv1d(self, x, w, *args, **kw):
        return TF.conv1d(x, w.to(x.dtype), *args, **kw)

    def conv_transpose1d(self, x, w, *args, **kw):
        return TF.conv_transpose1d(x, w.to(x.dtype), *args, **kw)


@contextlib.contextmanager
def float64_oracle():
    saved = ref_cpu.F
    ref_cpu.F = _FiltersInTheNetsDtype()
    try:
        yield
    finally:
        ref_cpu.F = saved


def _oracle(tag, mel):
    """-> (float64 oracle, float64-accumulated restatement of the bf16 mode, its distance (a) from the oracle, the fp32-accumulated
    restatement's distance (b) from it: tests/test_bf16_mode.py) of one clip"""
    sd, sd64 = state(tag)
    hp = CFGS[tag].as_hparams()
    with float64_oracle():
        ref = ref_cpu.bigvgan_forward(sd64, hp, mel.double())
    with bf16_mode(torch.float64):
        r64 = ref_cpu.bigvgan_forward(sd64, hp, mel.double())
    with bf16_mode(torch.float32):
        r32 = ref_cpu.bigvgan_forward(sd, hp, mel.float())
    return ref, r64, rel_l2(r64, ref), rel_l2(r32, r64)


@functools.lru_cache(maxsize=None)
def oracle_row(tag, b):
    """row b of MIXED on the clip alone; computed once, never modified"""
    T, lens = MIXED
    return _oracle(tag, mel_batch(T, len(lens))[b:b + 1, :, :lens[b]].contiguous())


def _hold(prec, wav, orc, what):
    """wav [1][1][n] against orc = _oracle(the clip), at the bound the suite holds BigVGAN to: rel-L2 < 5e-5 for fp32 / fp32mf and < 3e-4 for
    split (test_gpu_path.py::test_bigvgan_vs_golden_and_oracle); bf16 / bf16xt: the two-sided rule of test_gpu_bf16_mode.py with (a) and
    (b) of this clip - within 4 x (b) of the float64-accumulated restatement, within 1.25 x (a) of the oracle."""
    ref, r64, a, b = orc
    assert wav.shape == ref.shape
    e = rel_l2(wav, ref)
    if prec in ("fp32", "fp32mf", "split"):
        tol = 3e-4 if prec == "split" else 5e-5
        print(f"[{prec}] {what}: rel-L2 {e:.3e} ({tol:g})")
        assert e < tol, describe(f"{prec} {what} vs float64", wav, ref)
    else:
        er = rel_l2(wav, r64)
        print(f"[{prec}] {what}: vs restatement {er:.3e} (4 x {b:.3e}), vs float64 {e:.3e} (1.25 x {a:.3e})")
        assert er < 4 * b, describe(f"{prec} {what} vs restatement", wav, r64)
        assert e < 1.25 * a, describe(f"{prec} {what} vs float64", wav, ref)


@pytest.mark.parametrize("prog", PROGRAMS, ids=ids)
def test_mixed_residues_hold_the_precision_bound_like_the_clip_alone(nets, prog):
    T, lens = MIXED
    tag, prec = prog
    wav = nets[prog].vocode_lens(padded(T, lens), lens).cpu()
    for b, n in enumerate(lens):
        assert oracle_row(tag, b)[0].shape == (1, 1, n * HOP)
        _hold(prec, alone(nets, prog, T, len(lens), b, n), oracle_row(tag, b), f"{tag} clip {b} alone (length {n})")
        _hold(prec, wav[b:b + 1, :, :n * HOP], oracle_row(tag, b), f"{tag} row {b} of the lens call (length {n} of {T})")
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("prog", PROGRAMS, ids=ids)
def test_no_lengths_and_all_full_lengths_are_the_plain_call(nets, prog):
    net, B, T = nets[prog], 3, 24
    mel = mel_batch(T, B).cuda()
    plain = net.run(mel).cpu()
    assert torch.equal(net.vocode_lens(mel, None).cpu(), plain)
    assert torch.equal(net.vocode_lens(mel, [T] * B).cpu(), plain)
    lib = net.ctx.lib
    ws = torch.empty(lib.vb_bigvgan_lens_workspace_bytes(net.ctx.handle, B, T), dtype=torch.uint8, device="cuda")
    assert ws.numel() > lib.vb_net_workspace_bytes(net.ctx.handle, L.NET_VOCODER, B, T) + B * 80 * T * 4
    for lens in (None, L.Lens(None), L.Lens((C.c_int32 * B)(*[T] * B))):
        out = torch.full((B, 1, T * HOP), float("nan"), device="cuda")
        rc = lib.vb_bigvgan_forward_lens(net.ctx.handle, L.ptr(mel), B, T, C.byref(lens) if lens is not None else None, L.ptr(out), L.ptr(ws), L.stream_ptr())
        assert rc == 0, lib.vb_last_error()
        assert torch.equal(out.cpu(), plain)


def test_vocode_batch_is_vocode_lens_squeezed(nets):
    from versband_amd.model import VocoderBigVGAN
    T, lens = SAME_RESIDUE["mod0"]
    voc = object.__new__(VocoderBigVGAN)
    voc.net = lambda: nets[("amp1", "fp32mf")]
    wav = voc.vocode_batch(padded(T, lens), lengths=lens)
    assert wav.is_cuda and wav.shape == (len(lens), T * HOP)
    assert torch.equal(wav.cpu(), lens_run(nets, ("amp1", "fp32mf"), T, lens)[:, 0])


# ---------------------------------------------------------------------------------------------------------------- e
def test_refusals_name_the_row_or_the_limit_and_leave_wav_untouched(nets):
    net, T = nets[("amp1", "fp32mf")], 24
    lib = net.ctx.lib

    def call(lens):
        B = len(lens)
        mel = torch.zeros(B, 80, T, device="cuda")
        wav = torch.full((B, 1, T * HOP), 7.0, device="cuda")
        ws = torch.empty(max(256, lib.vb_bigvgan_lens_workspace_bytes(net.ctx.handle, B, T)), dtype=torch.uint8, device="cuda")
        ls = L.Lens((C.c_int32 * B)(*lens))
        rc = lib.vb_bigvgan_forward_lens(net.ctx.handle, L.ptr(mel), B, T, C.byref(ls), L.ptr(wav), L.ptr(ws), L.stream_ptr())
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
            net.vocode_lens(torch.zeros(len(lens), 80, T), lens)


def test_vae_nets_are_refused_by_name(ctx):
    from versband_amd.engine import build_vae_decoder, build_vae_encoder
    dec = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), SEED + 1), precision="fp32")
    with pytest.raises(ValueError, match="VAE decoder"):
        dec.vocode_lens(torch.zeros(2, dec.in_ch, 16), [16, 8])
    enc = build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(synth.VAEConfig()), SEED + 3), precision="fp32")
    with pytest.raises(ValueError, match="VAE encoder"):
        enc.vocode_lens(torch.zeros(2, enc.in_ch, 16 * enc.in_tmul), [16, 8])
    # through the ABI the decoder's context has no vocoder program: refused before anything runs, wav untouched
    lib, B, T = dec.ctx.lib, 2, 16
    wav = torch.full((B, 1, T * HOP), 7.0, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    ls = L.Lens((C.c_int32 * B)(16, 8))
    rc = lib.vb_bigvgan_forward_lens(dec.ctx.handle, L.ptr(torch.zeros(B, 80, T, device="cuda")), B, T, C.byref(ls), L.ptr(wav), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"no vocoder loaded" in lib.vb_last_error() and bool((wav == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("prog", PROGRAMS, ids=ids)
def test_chunked_rows_equal_run_chunked_on_the_clip_alone(nets, prog):
    T, chunk, halo, lens = CHUNKED
    net = nets[prog]
    steps = harness.plan_chunk_calls(lens, T, chunk, halo)
    assert [c["rows"] for c in steps] == [[0, 1, 2], [0, 1], [0]]          # rows 2 and 1 ended before the second / third chunk: not run there
    assert all(n % 4 == c["tc"] % 4 for c in steps for n in c["n"])
    # (each clip's own grid keeps the steps of this one: 12 frames are one step either way, 28 frames are chunked at 0 and 16)
    for b, n in enumerate(lens):
        own = harness.plan_chunk_calls([n], n, chunk, halo)
        mine = [(c["lo"], c["n"][c["rows"].index(b)]) for c in steps if b in c["rows"]]
        assert [(c["lo"], c["n"][0]) for c in own] == mine or (len(own) == 1 and mine == [(0, n)])
    wav = net.vocode_lens(padded(T, lens, float("nan")), lens, chunk=chunk, halo=halo).cpu()
    assert wav.shape == (len(lens), 1, T * HOP) and torch.isfinite(wav).all()
    for b, n in enumerate(lens):
        ref = net.run_chunked(mel_batch(T, len(lens))[b:b + 1, :, :n].contiguous(), chunk, halo).cpu()
        got = wav[b:b + 1, :, :n * HOP]
        assert torch.equal(got, ref), describe(f"{prog}: row {b} (length {n} of {T}) vs run_chunked on the clip alone", got, ref)
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0, f"{prog}: row {b} has nonzero samples behind its end"
        assert float(got.abs().max()) > 0
    full = net.vocode_lens(mel_batch(T, 2), [T, T], chunk=chunk, halo=halo).cpu()
    assert torch.equal(full, net.run_chunked(mel_batch(T, 2), chunk, halo).cpu())


def test_chunked_refusals_through_the_abi_leave_wav_untouched(nets):
    net = nets[("amp1", "fp32mf")]
    lib, h = net.ctx.lib, net.ctx.handle
    T, chunk, halo, _ = CHUNKED
    tc = chunk + 2 * halo
    for lens, text in (([40, 0, 12], b"row 1"), ([40, 41, 12], b"row 1")):
        B = len(lens)
        wav = torch.full((B, 1, T * HOP), 7.0, device="cuda")
        cin, cout = torch.empty(B * 80 * tc, device="cuda"), torch.empty(B * tc * HOP, device="cuda")
        ws = torch.empty(max(256, lib.vb_bigvgan_chunked_lens_workspace_bytes(h, B, T, chunk, halo)), dtype=torch.uint8, device="cuda")
        ls = L.Lens((C.c_int32 * B)(*lens))
        rc = lib.vb_bigvgan_forward_chunked_lens(h, L.ptr(torch.zeros(B, 80, T, device="cuda")), B, T, chunk, halo, C.byref(ls), L.ptr(wav), L.ptr(ws),
                                                 L.ptr(cin), L.ptr(cout), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and text in lib.vb_last_error() and bool((wav == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- g
UNIT_C, UNIT_T = 3, 600
UNIT_LENS = [600, 512, 257, 256, 255, 6, 1]      # the pitch; two tiles; the tile boundary and its neighbours; shorter than the filter's half; one sample


@functools.lru_cache(maxsize=None)
def unit_inputs():
    B = len(UNIT_LENS)
    x = torch.from_numpy(synth.prng.uniform(23, B * UNIT_C * UNIT_T, -3.0, 3.0).reshape(B, UNIT_C, UNIT_T).copy()).float()
    alpha = torch.tensor([0.6, 1.0, 1.7])
    beta = torch.tensor([1.3, 0.8, 0.5])
    return x, alpha, (1.0 / (beta + 1e-9)).float(), beta, pack.kaiser_sinc_filter1d(0.25, 0.3, 12).float()


def aa_reference(x, alpha, beta, inv_beta, f):
    """-> (ref, bound) float64 of the activation on whole rows x [B][C][n].  ref is ref_cpu.aa_activation in float64 on the kernel's own
    fp32 operands.  The bound is the rule tests/test_gpu_conv_units.py holds the exact-fp32 kernels to (tests/conv_oracles.py: fp32
    accumulation of K products in any order errs by acc(K) = 2 K U32 relative to sum |x_k| |w_k|, every further rounding by U32 of its
    result), carried through the kernel's three stages, first order:
      up   = 2 sum_6 xp f                          E_up = acc(6) S_up                                  (the doubling is exact)
      sn   = sinf(up a)                            E_sn = a E_up + U32 |up a| + 4 U32 |sn|             (|cos| <= 1; sinf to 2 ulp = 4 U32)
      s    = up + ib sn^2                          E_s  = E_up + ib (2 |sn| E_sn + U32 sn^2) + 3 U32 ib sn^2 + U32 |s|
                                                   (ib itself is the host's fp32 1 / (beta + 1e-9): two roundings, 2 U32; the product; the sum)
      out  = sum_12 f s                            E    = conv(E_s, |f|) + acc(12) conv(|s|, |f|)"""
    with float64_oracle():
        ref = ref_cpu.aa_activation(x.double(), alpha.double(), beta.double(), False)
    # (ib: the oracle's float64 1 / (beta + 1e-9); the kernel's fp32 inv_beta lies within 2 U32 of it, which E_s carries)
    x, a, ib, f = x.double(), alpha.double()[None, :, None], 1.0 / (beta.double()[None, :, None] + 1e-9), f.double()
    assert float((inv_beta.double()[None, :, None] / ib - 1).abs().max()) <= 2 * U32
    Cc = x.shape[1]
    w = f.view(1, 1, 12).expand(Cc, -1, -1)

    def up2(v, wt):
        return 2 * TF.conv_transpose1d(TF.pad(v, (5, 5), mode="replicate"), wt, stride=2, groups=Cc)[..., 15:-15]

    def down2(v, wt):
        return TF.conv1d(TF.pad(v, (5, 6), mode="replicate"), wt, stride=2, groups=Cc)

    up, e_up = up2(x, w), 2 * 6 * U32 * up2(x.abs(), w.abs())
    sn = torch.sin(up * a)
    e_sn = a * e_up + U32 * (up * a).abs() + 4 * U32 * sn.abs()
    s = up + ib * sn * sn
    e_s = e_up + ib * (2 * sn.abs() * e_sn + U32 * sn * sn) + 3 * U32 * ib * sn * sn + U32 * s.abs()
    mine = down2(s, w)
    assert float((mine - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), "the restatement the bound is built on is not the oracle's"
    return ref, down2(e_s, w.abs()) + 2 * 12 * U32 * down2(s.abs(), w.abs())


def aa_call(lib, x, alpha, inv_beta, f, lens=None, len_mul=1):
    xd = x.cuda().contiguous()
    B, Cc, T = xd.shape
    out = torch.full_like(xd, float("nan"))
    held = [alpha.cuda(), inv_beta.cuda(), f.cuda()]
    table = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
    L.check(lib.vb_aa_act(L.ptr(xd), L.ptr(held[0]), L.ptr(held[1]), L.ptr(held[2]), B, Cc, T, L.ptr(table) if table is not None else None, len_mul,
                          L.ptr(out), L.stream_ptr()), "vb_aa_act")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("len_mul", [1, 2])
def test_aa_act_unit_with_lengths(ctx, len_mul):
    x, alpha, inv_beta, beta, f = unit_inputs()
    rows = [b for b, n in enumerate(UNIT_LENS) if n % len_mul == 0]
    lens = [UNIT_LENS[b] for b in rows]
    assert lens == (UNIT_LENS if len_mul == 1 else [600, 512, 256, 6])
    xin = x[rows].clone()
    for j, n in enumerate(lens):
        xin[j, :, n:] = float("nan")                  # the input tail: never read
    got = aa_call(ctx.lib, xin, alpha, inv_beta, f, [n // len_mul for n in lens], len_mul)
    worst = 0.0
    for j, n in enumerate(lens):
        clip = x[rows[j]:rows[j] + 1, :, :n].contiguous()
        ref, bound = aa_reference(clip, alpha, beta, inv_beta, f)
        one = aa_call(ctx.lib, clip, alpha, inv_beta, f)
        assert torch.isfinite(one).all()
        assert torch.equal(got[j:j + 1, :, :n], one), describe(f"row {j} (length {n}) vs the kernel on the row alone", got[j:j + 1, :, :n], one)
        assert got[j, :, n:].numel() == UNIT_C * (UNIT_T - n) and int(torch.count_nonzero(got[j, :, n:])) == 0 and not torch.isnan(got[j, :, n:]).any()
        err = (one.double() - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), f"row {j} (length {n}): {int((err > bound).sum())} elements outside the bound, worst {float((err / bound).max()):.2f}x"
    print(f"vb_aa_act len_mul={len_mul}: worst err / bound = {worst:.3f}")
