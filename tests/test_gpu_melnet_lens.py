"""MelNet with row lengths on the GPU (vb_melnet_forward_lens, MelNet.forward(lengths=)), the masked mel distance (vb_mel_dist_lens,
melnet.mel_distance) and the --eval_mel tail of scripts/infer_batched.py that uses both.

The contract of include/versband_hip.h: row b's first T_b frames are the call on that clip alone BIT FOR BIT, always (the STFT convolution
runs one of two exact-fp32 kernels that accumulate in one order - tests/test_melnet_lens_host.py pins the routes: here the padded call and
the clips of 30, 16 and 2 frames take different ones), frames behind T_b are exact zeros and the padding of the waveform is never read.

Shapes (MEL_HP: n_fft 1280, hop 320, pad 480, 80 mels), L = 37 * 320: a full row; a ragged one (9607 samples, 30 frames); 16 frames = one
frame tile of both kernels exactly; 17 = one past it; 2 frames, where the reflection reaches almost across the row; 1 frame (481 samples),
the smallest legal row."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.test_oracle_golden import MEL_HP, mel_close
from versband_amd import _lib as L
from versband_amd import prng

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, PAD = 320, 480
LMAX = 37 * HOP
LENS = [11840, 9607, 5120, 5443, 641, 481]
LENS_CENTER = [11840, 5443, 1300]
U32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def net():
    from versband_amd.melnet import MelNet
    return MelNet(MEL_HP, device="cuda:0")


@functools.lru_cache(maxsize=None)
def clips(B):
    """B rows of LMAX samples, louder than full scale in places (the clamp acts); never modified"""
    t = np.arange(LMAX, dtype=np.float64) / 24000.0
    rows = [0.9 * np.sin(2 * np.pi * 220.0 * (b + 1) * t) * (0.5 + 0.8 * np.sin(2 * np.pi * 3.0 * t + b) ** 2) + 0.2 * prng.normal(500 + b, LMAX) for b in range(B)]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def padded(lens, fill):
    wav = clips(len(lens)).clone()
    for b, n in enumerate(lens):
        wav[b, n:] = fill
    return wav


@functools.lru_cache(maxsize=None)
def alone(lens, center, complex=False):
    """every clip through the plain call on its own: the reference of a row, computed once"""
    out = [net()(clips(len(lens))[b, :n], center=center, complex=complex)[0].cpu() for b, n in enumerate(lens)]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("center,lens", [(False, tuple(LENS)), (True, tuple(LENS_CENTER))], ids=["plain", "center"])
def test_rows_are_the_clip_alone_bit_for_bit_with_zeros_behind(center, lens):
    """1, 2, 3 and 5 of the issue: against the clip alone (bit for bit, every row), against the oracle on the clip alone (the bounds of
    tests/test_gpu_path.py::test_melnet_vs_golden_and_oracle: mel_close at 1e-3), exact zeros behind T_b, everything finite - with NaN
    behind every row's end"""
    m = net()
    wav = padded(lens, float("nan"))
    mel = m(wav, center=center, lengths=list(lens)).cpu()
    spec = m(wav, center=center, complex=True, lengths=list(lens)).cpu()
    T = m.frames(LMAX, center)
    assert mel.shape == (len(lens), 80, T) and spec.shape == (len(lens), T, 641, 2)
    assert torch.isfinite(mel).all() and torch.isfinite(spec).all()
    fb = m.mel_basis.cpu()
    for b, n in enumerate(lens):
        Tb = m.frames(n, center)
        one, one_spec = alone(lens, center)[b], alone(lens, center, True)[b]
        assert one.shape == (80, Tb)
        assert torch.equal(mel[b, :, :Tb], one), (b, n, float((mel[b, :, :Tb] - one).abs().max()))
        assert torch.equal(spec[b, :Tb], one_spec), (b, n, float((spec[b, :Tb] - one_spec).abs().max()))
        assert not mel[b, :, Tb:].any() and not spec[b, Tb:].any(), (b, n)
        ref = ref_cpu.melnet_forward(clips(len(lens))[b:b + 1, :n], MEL_HP, fb, center=center)[0]
        mel_close(mel[b, :, :Tb].numpy(), ref.numpy(), 1e-3)
    assert [m.frames(n) for n in LENS] == [37, 30, 16, 17, 2, 1]


def test_zero_padding_alone_gets_the_last_frames_wrong():
    """4: the feature matters at these shapes - the equal-length call on the zero-padded batch differs from the clip alone in the last frames
    of every short row (the reflection turns round at the call's end, not the row's)"""
    m = net()
    mel = m(padded(LENS, 0.0)).cpu()
    for b, n in enumerate(LENS):
        Tb, one = m.frames(n), alone(tuple(LENS), False)[b]
        if n == LMAX:
            assert torch.equal(mel[b], one)
        else:
            assert float((mel[b, :, Tb - 1] - one[:, Tb - 1]).abs().max()) > 1e-2, (b, n)


def test_no_lengths_and_full_lengths_are_the_plain_call():
    """6: lengths=None and all-full lengths return the plain call's bits"""
    m = net()
    wav = clips(3)
    for center in (False, True):
        plain = m(wav, center=center).cpu()
        assert torch.equal(m(wav, center=center, lengths=None).cpu(), plain)
        assert torch.equal(m(wav, center=center, lengths=[LMAX] * 3).cpu(), plain)
        assert torch.equal(m(wav, center=center, complex=True, lengths=[LMAX] * 3).cpu(), m(wav, center=center, complex=True).cpu())


def test_refusals_name_the_row():
    """7: a length of 480 (= pad), of 0, above L, and B + 1 lengths - from the Python host and from the library itself"""
    m = net()
    wav = clips(6)
    for lens, text in (([11840, 9607, 480, 5443, 641, 481], r"lengths\[2\] = 480"), ([11840, 0, 5120, 5443, 641, 481], r"lengths\[1\] = 0"),
                       ([11840, 9607, 5120, 11841, 641, 481], r"lengths\[3\] = 11841"), (LENS + [481], "7 entries for 6 rows")):
        with pytest.raises(ValueError, match=text):
            m(wav, lengths=lens)
    # the library's own checks, past the Python mirror: the row is named, nothing is launched, mel is unchanged
    lib, dev = m._ctx.lib, m._ctx.device
    y = wav.to(dev)
    mel = torch.full((6, 80, m.frames(LMAX, True)), 7.0, device=dev)           # (room for either geometry)
    ws = torch.empty(lib.vb_melnet_lens_workspace_bytes(C.byref(m._cfg), 6, LMAX, 1), dtype=torch.uint8, device=dev)
    for lens, ctr, text in (([11840, 9607, 480, 5443, 641, 481], 0, "row 2: reflect padding 480"), ([11840, 0, 5120, 5443, 641, 481], 0, "row 1 has length 0"),
                            ([11840, 9607, 5120, 11841, 641, 481], 0, "row 3 has length 11841"), ([11840, 9607, 5120, 5443, 481, 481], 0, None),
                            ([11840, 9607, 5120, 5443, 481, 480], 1, "row 5: reflect padding 480")):
        arr = (C.c_int32 * 6)(*lens)
        rc = lib.vb_melnet_forward_lens(m._ctx.handle, L.ptr(y), 6, LMAX, ctr, C.byref(L.Lens(arr)), L.ptr(mel), None, L.ptr(ws), L.stream_ptr())
        if text is None:
            assert rc == 0
            mel.fill_(7.0)
        else:
            assert rc == -1 and text in lib.vb_last_error().decode(), (lens, lib.vb_last_error())
            assert bool((mel == 7.0).all()), "a refused call leaves mel unchanged"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- mel_distance
DIST_FRAMES = [37, 16, 17, 1]


@functools.lru_cache(maxsize=None)
def dist_inputs():
    a = prng.uniform(71, 4 * 80 * 37, -5.0, 0.5).reshape(4, 80, 37).astype(np.float32)
    b = prng.uniform(72, 4 * 80 * 40, -5.0, 0.5).reshape(4, 80, 40).astype(np.float32)
    a[1] += np.float32(0.3)
    return a, b


def dist_ref(a, b, frames, remove_offset):
    out, off = [], []
    for r, f in enumerate(frames):
        d = a[r, :, :f].astype(np.float64) - b[r, :, :f].astype(np.float64)
        mu = d.mean() if remove_offset else 0.0
        out.append(np.abs(d - mu).mean())
        off.append(mu)
    return np.array(out), np.array(off)


@pytest.mark.parametrize("remove_offset", [False, True])
def test_mel_distance_against_float64_within_the_derived_bound(remove_offset):
    """The reduction shape (include/versband_hip.h, melnet.hip): a thread adds at most ceil(N / 1024) elements serially, then a 10-level LDS
    tree.  At M = 80 and 37 frames N = 2960: k = ceil(2960 / 1024) + 10 = 3 + 10 = 13 additions on the longest chain, and the bound is
    |dev - ref| <= 2 k 2^-24 (mean|d| + |mu|) = 1.55e-6 (mean|d| + |mu|) - about 3e-6 at the inputs' mean |d| of ~1.9.  The shorter rows
    have k = 12 (16 and 17 frames) and k = 11 (1 frame); each row is held to its own k.  Two calls return identical bits, and NaN behind
    frames[r] changes nothing."""
    from versband_amd.melnet import mel_distance
    a, b = dist_inputs()
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dist, off = mel_distance(ta, tb, DIST_FRAMES, remove_offset=remove_offset)
    dist2, off2 = mel_distance(ta, tb, DIST_FRAMES, remove_offset=remove_offset)
    assert dist.shape == off.shape == (4,) and dist.device == ta.device
    assert torch.equal(dist, dist2) and torch.equal(off, off2), "run-to-run identical"
    ref, ref_off = dist_ref(a, b, DIST_FRAMES, remove_offset)
    d_abs, _ = dist_ref(a, b, DIST_FRAMES, False)
    got, got_off = dist.cpu().double().numpy(), off.cpu().double().numpy()
    assert [-(-80 * f // 1024) + 10 for f in DIST_FRAMES] == [13, 12, 12, 11]
    for r, f in enumerate(DIST_FRAMES):
        k = -(-80 * f // 1024) + 10
        bound = 2 * k * U32 * (d_abs[r] + abs(ref_off[r]))
        print(f"row {r}: frames {f} k {k} dist err {abs(got[r] - ref[r]):.3e} offset err {abs(got_off[r] - ref_off[r]):.3e} bound {bound:.3e}")
        assert abs(got[r] - ref[r]) <= bound, (r, got[r], ref[r], bound)
        assert abs(got_off[r] - ref_off[r]) <= bound, (r, got_off[r], ref_off[r], bound)
    if remove_offset:
        assert abs(got_off[1] - got_off[0]) > 0.2, "the row with 0.3 added carries it in its offset"
    else:
        assert not got_off.any()
    an, bn = a.copy(), b.copy()
    for r, f in enumerate(DIST_FRAMES):
        an[r, :, f:] = np.nan
        bn[r, :, f:] = np.nan
    dn, on = mel_distance(torch.from_numpy(an).cuda(), torch.from_numpy(bn).cuda(), DIST_FRAMES, remove_offset=remove_offset)
    assert torch.equal(dn, dist) and torch.equal(on, off), "nothing behind frames[r] is read"
    for frames, text in (([37, 16, 38, 1], r"frames\[2\] = 38"), ([37, 0, 17, 1], r"frames\[1\] = 0"), ([37, 16, 17], "3 entries for 4 rows")):
        with pytest.raises(ValueError, match=text):
            mel_distance(ta, tb, frames)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_eval_mel_scores_a_group_together(tmp_path, monkeypatch):
    """scripts/infer_batched.py --synthetic 5 --synthetic_frames 64,48,56 --items_per_batch 4 --length_slack 16 --eval_mel, in process: a
    group of four clips of three lengths and a group of one.  mel_l1.tsv keeps its header, row count and order, and every value equals the
    per-clip formula - float64, from the waveform as written (before its PCM rounding: what the per-clip path analyses) through MelNet on that
    clip alone, and the decoded mel - within 2 k 2^-24 (mean|d| + |mu|), k = ceil(80 f / 1024) + 10 = 15 / 14 / 15 at 64 / 48 / 56 frames."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import infer_batched as ib
    written, decoded = {}, []
    real_write, real_sample = ib.write_wav_pcm16, ib.sample_group

    def write(path, wav, rate):
        written[os.path.basename(path)] = np.asarray(wav, dtype=np.float32).copy()
        return real_write(path, wav, rate)

    def sample(args, sampler, vocoder, group, scales, device):
        out = real_sample(args, sampler, vocoder, group, scales, device)
        for p in range(len(group)):
            for s in scales:
                decoded.extend(spec.detach().cpu() for spec, _ in out[(p, s)])
        return out

    monkeypatch.setattr(ib, "write_wav_pcm16", write)
    monkeypatch.setattr(ib, "sample_group", sample)
    args = ib.parse_args(["--synthetic", "5", "--synthetic_frames", "64,48,56", "--items_per_batch", "4", "--length_slack", "16", "--eval_mel",
                          "--ddim_steps", "1", "--scales", "3", "--n_samples", "1", "--save_dir", str(tmp_path)])
    ib.gen_song(0, args)
    lines = open(tmp_path / "mel_l1.tsv").read().splitlines()
    assert lines[0].split("\t") == ["name", "scale", "sample", "mel_l1_vs_decoded", "mel_l1_vs_gt_accomp"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [r[0] for r in rows] == [f"synthetic{i:04d}" for i in range(5)] and len(decoded) == 5
    frames = [64, 48, 56, 64, 48]
    m = net()
    for i, row in enumerate(rows):
        wav = written[f"0-{i:04d}[0][accomp].wav"]
        assert wav.shape == (frames[i] * HOP,) and decoded[i].shape == (80, frames[i])
        back = m(wav)[0].cpu().double().numpy()
        f = min(back.shape[1], decoded[i].shape[1])
        d = back[:, :f] - decoded[i][:, :f].double().numpy()
        ref, k = np.abs(d - d.mean()).mean(), -(-80 * f // 1024) + 10
        bound = 2 * k * U32 * (np.abs(d).mean() + abs(d.mean()))
        print(f"clip {i}: frames {f} k {k} value {float(row[3]):.9g} ref {ref:.9g} err {abs(float(row[3]) - ref):.3e} bound {bound:.3e}")
        assert float(row[1]) == 3.0 and int(row[2]) == 0
        assert abs(float(row[3]) - ref) <= bound, (i, row[3], ref, bound)          # (the tsv prints a float's shortest exact form)
        assert row[4] == "", "synthetic items have no ground truth"
