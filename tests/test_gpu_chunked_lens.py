"""The chunked vocoder with row lengths on the GPU (vb_hifigan_forward_chunked_lens, ConvNet.run_chunked(lengths=),
longform.vocode_chunked(lengths=), longform.render_long): long mels of different lengths as rows of one chunked call.  The contract of
include/versband_hip.h: row b's first len[b] * hop samples are the chunk loop over that clip alone on the same grid - bit for bit in every
chunk where the row's frames and the chunk's width agree mod 4, to fp32 roundoff elsewhere - the rest of the row is exact zeros, a row that
ended before a chunk is not run in it, and the mel padding is never read.

The generator is the one of tests/test_gpu_vocoder_lens.py (upsample_initial_channel = 256: unfused convolutions and fused 32- / 64-channel
pairs) in the five precisions.  MAIN: T = 56, chunk = 16, halo = 16 gives four chunks with 7 / 5 / 4 / 2 active rows; rows end inside a chunk,
inside a trailing halo and before a chunk begins; the last two chunks are narrower than chunk + 2 halo; every length is a multiple of 4.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, describe, rel_l2
from tests.test_bf16_mode import bf16_mode
from tests.test_gpu_vocoder_lens import CFG, HOP, PRECISIONS, _hold, mel_batch, padded, state
from versband_amd import _lib as L
from versband_amd import harness, longform, synth

pytestmark = pytest.mark.gpu
MAIN = (56, 16, 16, [56, 52, 40, 36, 20, 12, 4])
MIXED = (54, 16, 16, [54, 47, 33, 21, 9])
GUARD = 4096                      # floats on either side of a guarded buffer (a multiple of 4: the buffer keeps the allocation's alignment)
SENTINEL = 7.0


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


def guarded(n, fill=SENTINEL):
    """(whole allocation, the n floats between its two guard bands)"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def raw_call(net, mel, chunk, halo, lens, lens_struct=None):
    """vb_hifigan_forward_chunked_lens through the C ABI with caller-owned buffers: scratch_in, scratch_out and wav sized exactly as the
    header says, each between guard bands; wav pre-filled with the sentinel.  Returns (rc, message, wav on the host, guards intact)."""
    lib, h = net.ctx.lib, net.ctx.handle
    B, Cin, T = mel.shape
    tc = chunk + 2 * halo
    n_in, n_out, n_wav = B * Cin * max(tc, 1), B * net.out_ch * max(tc, 1) * HOP, B * net.out_ch * T * HOP
    (bi, cin), (bo, cout), (bw, wav) = guarded(n_in), guarded(n_out), guarded(n_wav)
    ws = torch.empty(max(256, lib.vb_hifigan_chunked_lens_workspace_bytes(h, B, T, chunk, halo),
                         lib.vb_net_workspace_bytes(h, L.NET_VOCODER, B, min(T, max(tc, 1)))), dtype=torch.uint8, device="cuda")
    if lens_struct is None and lens is not None:
        lens_struct = L.Lens((C.c_int32 * B)(*lens))
    rc = lib.vb_hifigan_forward_chunked_lens(h, L.ptr(mel), B, T, chunk, halo, C.byref(lens_struct) if lens_struct is not None else None,
                                             L.ptr(wav), L.ptr(ws), L.ptr(cin), L.ptr(cout), L.stream_ptr())
    torch.cuda.synchronize()
    ok = guards_intact(bi, n_in) and guards_intact(bo, n_out) and guards_intact(bw, n_wav)
    return rc, lib.vb_last_error(), wav.view(B, net.out_ch, T * HOP).cpu(), ok


_cache = {}


def lens_call(nets, prec, case):
    """the zero-padded call with lengths through the C ABI, once per (precision, case): (wav, guards intact)"""
    T, chunk, halo, lens = case
    key = (prec, T, chunk, halo, tuple(lens))
    if key not in _cache:
        rc, msg, wav, ok = raw_call(nets[prec], padded(T, lens).cuda(), chunk, halo, lens)
        assert rc == 0, msg
        _cache[key] = (wav, ok)
    return _cache[key]


def alone_loop(net, clip, chunk, halo, T):
    """the test's own chunk loop over one clip [1][80][n] on the grid of a T-frame call: per chunk the plain run of the clip's frames
    [lo, min(n, s + chunk + halo)), of which the samples of [s, min(e, n)) are kept"""
    n = clip.shape[2]
    if T <= chunk + 2 * halo:          # (the grid's one-step rule: the whole clip)
        return net.run(clip.contiguous()).cpu()
    out = torch.empty(1, 1, n * HOP)
    for s in range(0, T, chunk):
        if s >= n:
            break
        e, lo, hi = min(s + chunk, T, n), max(0, s - halo), min(n, s + chunk + halo)
        w = net.run(clip[:, :, lo:hi].contiguous()).cpu()
        out[:, :, s * HOP:e * HOP] = w[:, :, (s - lo) * HOP:(e - lo) * HOP]
    return out


def test_the_cases_are_what_the_docstring_says():
    T, chunk, halo, lens = MAIN
    steps = harness.plan_chunk_calls(lens, T, chunk, halo)
    assert [len(c["rows"]) for c in steps] == [7, 5, 4, 2] and [c["tc"] for c in steps] == [32, 48, 40, 24]
    assert all(n % 4 == c["tc"] % 4 for c in steps for n in c["n"])
    assert any(c["s"] < n < c["e"] for c in steps for n in lens) and any(c["e"] < n < c["e"] + halo for c in steps for n in lens)
    T, chunk, halo, lens = MIXED
    assert any(n % 4 != c["tc"] % 4 for c in harness.plan_chunk_calls(lens, T, chunk, halo) for n in c["n"])


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("prec", PRECISIONS)
def test_rows_equal_the_chunk_loop_over_the_clip_alone_bit_for_bit(nets, prec):
    T, chunk, halo, lens = MAIN
    wav, ok = lens_call(nets, prec, MAIN)
    assert ok, f"{prec}: a guard band of scratch_in / scratch_out / wav was written"
    assert wav.shape == (len(lens), 1, T * HOP) and torch.isfinite(wav).all()
    for b, n in enumerate(lens):
        ref = alone_loop(nets[prec], mel_batch(T, len(lens))[b:b + 1, :, :n], chunk, halo, T)
        got = wav[b:b + 1, :, :n * HOP]
        assert torch.equal(got, ref), describe(f"{prec}: row {b} (length {n} of {T}) vs the chunk loop over the clip alone", got, ref)
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0, f"{prec}: row {b} has nonzero samples behind its end"
        assert float(got.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("prec", PRECISIONS)
def test_each_chunk_equals_the_lengths_call_on_the_gathered_batch(nets, prec):
    T, chunk, halo, lens = MAIN
    wav, _ = lens_call(nets, prec, MAIN)
    mel = mel_batch(T, len(lens))
    for c in harness.plan_chunk_calls(lens, T, chunk, halo):
        x = torch.zeros(len(c["rows"]), 80, c["tc"])
        for j, (b, n) in enumerate(zip(c["rows"], c["n"])):
            x[j, :, :n] = mel[b, :, c["lo"]:c["lo"] + n]
        w = nets[prec].run(x, lengths=c["n"]).cpu()
        for j, b in enumerate(c["rows"]):
            e = min(c["e"], lens[b])
            got, ref = wav[b, :, c["s"] * HOP:e * HOP], w[j, :, (c["s"] - c["lo"]) * HOP:(e - c["lo"]) * HOP]
            assert torch.equal(got, ref), describe(f"{prec}: chunk at {c['s']}, row {b} vs run(lengths=) on the gathered batch", got, ref)


# ---------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_padding_is_never_read(nets, prec, fill):
    T, chunk, halo, lens = MAIN
    wav = nets[prec].run_chunked(padded(T, lens, fill), chunk, halo, lengths=lens).cpu()
    assert torch.isfinite(wav).all(), f"{prec}: padding of {fill} reached the output"
    assert torch.equal(wav, lens_call(nets, prec, MAIN)[0]), f"{prec}: the result depends on the mel padding"


# ---------------------------------------------------------------------------------------------------------------- d
@functools.lru_cache(maxsize=None)
def oracle_loop(b):
    """float64 oracle of row b of MIXED - the chunk loop on the clip alone - and the bf16 mode's restatement of it, float64- and
    fp32-accumulated (tests/test_bf16_mode.py); the tuple _hold takes.  Computed once, never modified."""
    T, chunk, halo, lens = MIXED
    n = lens[b]
    clip = mel_batch(T, len(lens))[b:b + 1, :, :n]
    sd, sd64 = state()
    hp = CFG.as_hparams()
    ref, r64, r32 = (torch.empty(1, 1, n * HOP, dtype=dt) for dt in (torch.float64, torch.float64, torch.float32))
    for s in range(0, min(T, n), chunk):
        e, lo, hi = min(s + chunk, n), max(0, s - halo), min(n, s + chunk + halo)
        piece = clip[:, :, lo:hi].contiguous()
        keep = slice((s - lo) * HOP, (e - lo) * HOP)
        ref[:, :, s * HOP:e * HOP] = ref_cpu.hifigan_forward(sd64, hp, piece.double())[:, :, keep]
        with bf16_mode(torch.float64):
            r64[:, :, s * HOP:e * HOP] = ref_cpu.hifigan_forward(sd64, hp, piece.double())[:, :, keep]
        with bf16_mode(torch.float32):
            r32[:, :, s * HOP:e * HOP] = ref_cpu.hifigan_forward(sd, hp, piece.float())[:, :, keep]
    return ref, r64, rel_l2(r64, ref), rel_l2(r32, r64)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_mixed_residues_hold_the_precision_bound_of_the_clip_alone(nets, prec):
    T, chunk, halo, lens = MIXED
    wav = nets[prec].run_chunked(padded(T, lens), chunk, halo, lengths=lens).cpu()
    for b, n in enumerate(lens):
        assert oracle_loop(b)[0].shape == (1, 1, n * HOP)
        _hold(prec, wav[b:b + 1, :, :n * HOP], oracle_loop(b), f"row {b} of the chunked lens call (length {n} of {T})")
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("prec", PRECISIONS)
def test_no_lengths_and_all_full_lengths_are_the_plain_chunked_call(nets, prec):
    net, B, (T, chunk, halo, _) = nets[prec], 3, MAIN
    mel = mel_batch(T, B).cuda()
    plain = net.run_chunked(mel, chunk, halo).cpu()
    assert torch.equal(net.run_chunked(mel, chunk, halo, lengths=[T] * B).cpu(), plain)
    assert torch.equal(longform.vocode_chunked(net, mel, chunk, halo, lengths=[T] * B).cpu(), plain)
    for lens_struct in (None, L.Lens(None), L.Lens((C.c_int32 * B)(*[T] * B))):
        rc, msg, wav, ok = raw_call(net, mel, chunk, halo, None, lens_struct)
        assert rc == 0 and ok, msg
        assert torch.equal(wav, plain)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_short_batches_are_the_whole_row_lengths_call(nets, prec):
    net, T, lens = nets[prec], 48, [48, 44, 20, 4]                  # T = chunk + 2 halo
    mel = padded(T, lens)
    whole = net.run(mel, lengths=lens).cpu()
    assert torch.equal(net.run_chunked(mel, 16, 16, lengths=lens).cpu(), whole)
    rc, msg, wav, ok = raw_call(net, mel.cuda(), 16, 16, lens)
    assert rc == 0 and ok, msg
    assert torch.equal(wav, whole)


# ---------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("prec", ["fp32", "fp32mf", "split"])
def test_chunked_equals_whole_vocoding_with_lengths(nets, prec):
    """halo 32 is far above the generator's ~14-frame receptive field; the bound and its cause are those of
    tests/test_gpu_configs.py::test_c5_vocoder_chunks_equal_whole: windows and whole rows may take different fp32 routes"""
    net, T, chunk, halo, lens = nets[prec], 120, 40, 32, [120, 96, 44]
    mel = padded(T, lens)
    whole = net.run(mel, lengths=lens).cpu()
    chunked = net.run_chunked(mel, chunk, halo, lengths=lens).cpu()
    assert chunked.shape == whole.shape
    for b, n in enumerate(lens):
        d = float((chunked[b, :, :n * HOP] - whole[b, :, :n * HOP]).abs().max())
        print(f"[{prec}] row {b} (length {n}): chunked vs whole max-abs {d:.3e} (2e-6)")
        assert d < 2e-6, describe(f"{prec}: row {b} chunked vs whole with lengths", chunked[b, :, :n * HOP], whole[b, :, :n * HOP])
        assert int(torch.count_nonzero(chunked[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- g
def test_refusals_name_the_row_or_the_limit_and_leave_wav_untouched(nets):
    net, T = nets["fp32mf"], 24

    def call(lens, chunk=8, halo=4):
        rc, msg, wav, ok = raw_call(net, torch.zeros(len(lens), 80, T, device="cuda"), chunk, halo, lens)
        assert ok and bool((wav == SENTINEL).all()), "a refused call must not touch wav"
        return rc, msg

    rc, msg = call([24, 0, 12])
    assert rc == -1 and b"row 1" in msg and b"length 0" in msg
    rc, msg = call([24, 12, 25])
    assert rc == -1 and b"row 2" in msg and b"length 25" in msg
    rc, msg = call([12] * 65)
    assert rc == -1 and b"65 rows" in msg and b"1..64" in msg
    rc, msg = call([24, 12], chunk=0)
    assert rc == -1 and b"chunk=0" in msg
    rc, msg = call([24, 12], halo=-1)
    assert rc == -1 and b"halo=-1" in msg
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0"), ([24, 12, 25], r"lengths\[2\] = 25"), ([12] * 65, "65 rows")):
        with pytest.raises(ValueError, match=text):
            net.run_chunked(torch.zeros(len(lens), 80, T), 8, 4, lengths=lens)


def test_no_vocoder_loaded_is_refused(ctx):
    from versband_amd.engine import Context
    bare = Context(ctx.device)
    wav = torch.full((2, 1, 24 * HOP), SENTINEL, device="cuda")
    mel, buf = torch.zeros(2, 80, 24, device="cuda"), torch.zeros(1 << 16, device="cuda")
    lens = L.Lens((C.c_int32 * 2)(24, 12))
    rc = bare.lib.vb_hifigan_forward_chunked_lens(bare.handle, L.ptr(mel), 2, 24, 8, 4, C.byref(lens), L.ptr(wav), L.ptr(buf), L.ptr(buf), L.ptr(buf), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"no vocoder loaded" in bare.lib.vb_last_error() and bool((wav == SENTINEL).all())
    assert bare.lib.vb_hifigan_chunked_lens_workspace_bytes(bare.handle, 2, 24, 8, 4) == 0


def test_bigvgan_as_the_vocoder_is_refused_naming_the_op(ctx):
    from tests.test_bf16_mode import fixture_case
    from versband_amd.engine import build_bigvgan
    sd, cfg, x, _, _ = fixture_case("bigvgan_amp1")
    net = build_bigvgan(ctx, sd, cfg.as_hparams(), precision="fp32")
    assert net.which == L.NET_VOCODER
    B, _, T = x.shape
    assert T >= 8
    chunk, halo = T // 4, 0                    # T > chunk + 2 halo: the chunked path, not the whole-row shortcut
    first = next(i for i, op in enumerate(net.nb.ops) if op.kind == L.OP_AA_ACT)
    lib, h = net.ctx.lib, net.ctx.handle
    mel = torch.cat([x, x]).cuda().float().contiguous()
    wav = torch.full((2 * B, net.out_ch, T * net.out_tmul), SENTINEL, device="cuda")
    ws = torch.empty(max(256, lib.vb_hifigan_chunked_lens_workspace_bytes(h, 2 * B, T, chunk, halo)), dtype=torch.uint8, device="cuda")
    cin = torch.empty(2 * B * net.in_ch * chunk, device="cuda")
    cout = torch.empty(2 * B * net.out_ch * chunk * net.out_tmul, device="cuda")
    lens = L.Lens((C.c_int32 * (2 * B))(*([T] * (2 * B - 1) + [T - 4])))
    rc = lib.vb_hifigan_forward_chunked_lens(h, L.ptr(mel), 2 * B, T, chunk, halo, C.byref(lens), L.ptr(wav), L.ptr(ws), L.ptr(cin), L.ptr(cout), L.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.vb_last_error().decode()
    assert rc == -1 and f"op {first} (VB_OP_AA_ACT)" in msg and "replicate-pad" in msg and bool((wav == SENTINEL).all())
    with pytest.raises(L.VersbandError) as e:
        net.run_chunked(mel, chunk, halo, lengths=[T] * (2 * B - 1) + [T - 4])
    assert f"op {first} (VB_OP_AA_ACT)" in str(e.value)


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("prec", ["fp32mf", "bf16xt"])
def test_one_row_and_sixty_four_rows_run(nets, prec, B):
    """short rows at T = 24, chunk = 8, halo = 4: three chunks; lengths are multiples of 4 like chunk, halo and T, so every row is
    bit-equal to the chunk loop over the clip alone.  One row: the padded T is longer than the row, the last chunk has no active row."""
    T, chunk, halo = 24, 8, 4
    lens = [12] if B == 1 else [24] + [4 * (1 + (5 * b) % 6) for b in range(1, B)]
    rc, msg, wav, ok = raw_call(nets[prec], padded(T, lens).cuda(), chunk, halo, lens)
    assert rc == 0 and ok, msg
    assert torch.isfinite(wav).all()
    for b, n in enumerate(lens):
        ref = alone_loop(nets[prec], mel_batch(T, B)[b:b + 1, :, :n], chunk, halo, T)
        assert torch.equal(wav[b:b + 1, :, :n * HOP], ref), describe(f"{prec}: row {b} of {B} (length {n})", wav[b:b + 1, :, :n * HOP], ref)
        assert int(torch.count_nonzero(wav[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- h
@pytest.mark.parametrize("prec", ["fp32mf", "bf16xt"])
def test_a_four_byte_aligned_mel_of_odd_length_gives_the_aligned_bits(nets, prec):
    """T = 55 and a base one float behind a 16-byte boundary: the gather's 4-byte path.  The same rows in an aligned T = 56 batch (same
    chunk grid, same in-chunk lengths) take the 16-byte path; the rows' own samples hold the same bits, and so does the aligned T = 55."""
    net, chunk, halo, lens = nets[prec], 16, 16, [55, 52, 40, 23]
    B = len(lens)
    src = mel_batch(56, B)
    odd = src[:, :, :55].contiguous()
    flat = torch.full((B * 80 * 55 + 4,), float("nan"), device="cuda")
    shifted = flat[1:1 + B * 80 * 55].view(B, 80, 55)
    shifted.copy_(odd)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    rc, msg, wav_shift, ok = raw_call(net, shifted, chunk, halo, lens)
    assert rc == 0 and ok, msg
    rc, msg, wav_odd, ok = raw_call(net, odd.cuda(), chunk, halo, lens)
    assert rc == 0 and ok, msg
    assert torch.equal(wav_shift, wav_odd), f"{prec}: the result depends on the mel's alignment"
    even = src.cuda()
    assert even.data_ptr() % 16 == 0
    rc, msg, wav_even, ok = raw_call(net, even, chunk, halo, lens)
    assert rc == 0 and ok, msg
    for b, n in enumerate(lens):
        assert torch.equal(wav_shift[b, :, :n * HOP], wav_even[b, :, :n * HOP]), f"{prec}: row {b} differs between the 4-byte and the 16-byte gather"
        assert int(torch.count_nonzero(wav_shift[b, :, n * HOP:])) == 0 and int(torch.count_nonzero(wav_even[b, :, n * HOP:])) == 0


# ---------------------------------------------------------------------------------------------------------------- i
def test_render_long_equals_decode_and_chunk_loop_on_each_clip_alone(ctx, nets):
    from versband_amd.engine import build_vae_decoder
    vcfg = synth.VAEConfig(ch=32)
    vae = build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(vcfg), SEED + 1), precision="fp32")
    T, lens = 16, [16, 12, 8]
    z = torch.from_numpy(synth.prng.normal(83, 3 * vae.in_ch * T).reshape(3, vae.in_ch, T).copy()).float()
    zp = z.clone()
    for b, n in enumerate(lens):
        zp[b, :, n:] = float("nan")
    # chunk = halo = 16: the 32 mel frames of the longest clip are one step (the whole rows); chunk 8, halo 4: four chunks on the grid of
    # the 32-frame batch, which the clip alone is looped over as well
    for prec, chunk, halo in (("fp32mf", 16, 16), ("bf16xt", 16, 16), ("fp32mf", 8, 4), ("bf16xt", 8, 4)):
        voc = nets[prec]
        wavs = longform.render_long(vae, voc, zp, lens, chunk=chunk, halo=halo)
        assert len(wavs) == 3
        for b, n in enumerate(lens):
            mel = vae.run(z[b:b + 1, :, :n].contiguous())
            assert mel.shape[2] == n * vae.out_tmul
            ref = alone_loop(voc, mel.cpu(), chunk, halo, T * vae.out_tmul)
            got = wavs[b].cpu()
            assert got.shape == (1, n * vae.out_tmul * HOP)
            assert torch.equal(got, ref[0]), describe(f"{prec}: render_long clip {b} ({n} tokens) vs decode + chunk loop alone", got, ref[0])
        both = longform.render_long(vae, voc, z, None, chunk=chunk, halo=halo)
        assert torch.equal(both, longform.vocode_chunked(voc, vae.run(z), chunk, halo))
