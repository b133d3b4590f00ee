"""MelNet with row lengths and the masked mel distance, host side (no GPU): the declarations and their binding, the refusals the library
decides before any launch, the route facts the bit-for-bit contract rests on (vb_conv1d_plan) and a numpy restatement of the framing
kernel's two-reflection index with a per-row length against the oracle on the clip alone.  The GPU half is tests/test_gpu_melnet_lens.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.test_oracle_golden import MEL_HP
from versband_amd import _lib as L
from versband_amd import prng
from versband_amd.melnet import MelNet, mel_filterbank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FFT, HOP, PAD = MEL_HP["fft_size"], MEL_HP["hop_size"], (MEL_HP["fft_size"] - MEL_HP["hop_size"]) // 2
TAPS = N_FFT // HOP
LENS = [11840, 9607, 5120, 5443, 641, 481]          # the rows of the GPU test: full, ragged, one frame tile, one past it, 2 frames, 1 frame
LENS_CENTER = [11840, 5443, 1300]


def frames_of(n, center):
    p = PAD + (N_FFT // 2 if center else 0)
    return 1 + (n + 2 * p - N_FFT) // HOP


def frames_index(L, Lb, center):
    """frames_kernel's index arithmetic with a length table, restated: for a row of Lb samples in a call padded to L, the sample every
    (hop-block j < J, channel c) reads, or -1 where the kernel writes a zero without loading (j >= J_b)"""
    pad2 = N_FFT // 2 if center else 0
    J, Jb = frames_of(L, center) + TAPS - 1, (Lb + 2 * (PAD + pad2) - N_FFT) // HOP + TAPS
    L1 = Lb + 2 * PAD
    k = np.arange(J * HOP, dtype=np.int64) - pad2
    k = np.abs(k)
    k = np.where(k >= L1, 2 * (L1 - 1) - k, k)
    k = np.abs(k - PAD)
    k = np.where(k >= Lb, 2 * (Lb - 1) - k, k)
    live = np.arange(J * HOP) < Jb * HOP
    assert k[live].min() >= 0 and k[live].max() < Lb, "a live block reads inside the row's own samples (the final clamp never acts)"
    return np.where(live, k, -1).reshape(J, HOP), Jb


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_new_entry_points_are_declared_bound_and_additive():
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for ret, name in (("size_t", "vb_melnet_lens_workspace_bytes"), ("int", "vb_melnet_forward_lens"), ("size_t", "vb_mel_dist_workspace_bytes"),
                      ("int", "vb_mel_dist_lens")):
        args = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (ret, name), code)
        assert args, name
        assert len(args.group(1).split(",")) == len(L.PROTOTYPES[name][1]), name
    assert L.PROTOTYPES["vb_melnet_forward_lens"][1][5] == C.POINTER(L.Lens)
    plain, lens = L.PROTOTYPES["vb_melnet_forward"][1], L.PROTOTYPES["vb_melnet_forward_lens"][1]
    assert lens[:5] == plain[:5] and lens[6:] == plain[5:], "the plain call's arguments with the vb_lens block after `center`"
    lib = L.load()
    assert all(hasattr(lib, n) for n in ("vb_melnet_lens_workspace_bytes", "vb_melnet_forward_lens", "vb_mel_dist_workspace_bytes", "vb_mel_dist_lens"))
    assert lib.vb_abi_version() == 3
    doc = src[src.index("The front-end with ROW LENGTHS"):src.index("int vb_mel_dist_lens(")]
    for needle in ("vb_melnet_forward on that clip alone", "exact zero", "is not read", "BIT FOR BIT, ALWAYS", "VB_ROUTE_F32G / VB_ROUTE_F32", "names the row",
                   "k = ceil(N / 1024) + 10", "identical from run to run", "no atomics"):
        assert needle in doc, needle


def test_workspace_sizes():
    lib = L.load()
    cfg = L.MelConfig(N_FFT, HOP, 80)
    plain = lib.vb_melnet_workspace_bytes(C.byref(cfg), 6, 11840, 0)
    assert lib.vb_melnet_lens_workspace_bytes(C.byref(cfg), 6, 11840, 0) == plain + 2 * 256, "the plain workspace and two tables of 64 lengths"
    assert lib.vb_melnet_lens_workspace_bytes(None, 6, 11840, 0) == 0
    assert lib.vb_mel_dist_workspace_bytes(1) == lib.vb_mel_dist_workspace_bytes(64) == 256
    assert lib.vb_mel_dist_workspace_bytes(0) == 0 and lib.vb_mel_dist_workspace_bytes(65) == 0


# ---------------------------------------------------------------------------------------------------------------- refusals before any launch
def i32(v):
    return (C.c_int32 * len(v))(*v)


def test_melnet_forward_lens_refuses_a_bad_row_on_the_host():
    """the lengths go through lens_plan before anything else: a bad row comes back as VB_E_INVALID with the row named - without a GPU,
    without a context, and without wav / mel being touched (host pointers would fault if they were)"""
    lib = L.load()
    wav, mel, ws = np.zeros((3, 6400), np.float32), np.zeros((3, 80, 20), np.float32), np.zeros(64, np.float32)
    pw, pm, pws = (x.ctypes.data_as(C.c_void_p) for x in (wav, mel, ws))
    for lens, B, pat in (([6400, 0, 3200], 3, "row 1 has length 0"), ([6400, 3200, 6401], 3, "row 2 has length 6401"), ([-5, 1, 1], 3, "row 0 has length -5"),
                         ([3200] * 65, 65, "row 64")):
        arr = i32(lens)
        rc = lib.vb_melnet_forward_lens(None, pw, B, 6400, 0, C.byref(L.Lens(arr)), pm, None, pws, None)
        assert rc == -1 and pat in lib.vb_last_error().decode(), (lens, rc, lib.vb_last_error())
    # lengths in range: the next thing missing is the loaded front-end (VB_E_STATE), with and without lengths
    arr = i32([6400, 3200, 481])
    rc_lens = lib.vb_melnet_forward_lens(None, pw, 3, 6400, 0, C.byref(L.Lens(arr)), pm, None, pws, None)
    assert rc_lens != 0 and rc_lens != -1 and b"not loaded" in lib.vb_last_error()
    assert lib.vb_melnet_forward_lens(None, pw, 3, 6400, 0, None, pm, None, pws, None) == rc_lens == lib.vb_melnet_forward(None, pw, 3, 6400, 0, pm, None, pws, None)
    assert not wav.any() and not mel.any()


def test_mel_dist_lens_refuses_on_the_host():
    lib = L.load()
    a, b, out, ws = np.zeros((4, 80, 37), np.float32), np.zeros((4, 80, 40), np.float32), np.zeros(4, np.float32), np.zeros(64, np.float32)
    pa, pb, po, pws = (x.ctypes.data_as(C.c_void_p) for x in (a, b, out, ws))
    for frames, B, pat in (([37, 16, 38, 1], 4, "row 2 has length 38"), ([37, 0, 17, 1], 4, "row 1 has length 0"), ([1] * 65, 65, "row 64")):
        rc = lib.vb_mel_dist_lens(pa, 37, pb, 40, B, 80, i32(frames), 0, po, None, pws, None)
        assert rc == -1 and pat in lib.vb_last_error().decode(), (frames, lib.vb_last_error())
    ok = i32([37, 16, 17, 1])
    assert lib.vb_mel_dist_lens(pa, 37, pb, 40, 4, 80, None, 0, po, None, pws, None) == -1 and b"len is null" in lib.vb_last_error()
    for args in ((None, 37, pb, 40, 4, 80, ok, 0, po, None, pws, None), (pa, 37, None, 40, 4, 80, ok, 0, po, None, pws, None),
                 (pa, 37, pb, 40, 4, 80, ok, 0, None, None, pws, None), (pa, 37, pb, 40, 4, 80, ok, 0, po, None, None, None),
                 (pa, 0, pb, 40, 4, 80, ok, 0, po, None, pws, None), (pa, 37, pb, 40, 4, 0, ok, 0, po, None, pws, None)):
        assert lib.vb_mel_dist_lens(*args) == -1 and b"mel_dist_lens" in lib.vb_last_error()
    assert not out.any()


def test_python_checks_name_the_row():
    from versband_amd.melnet import mel_distance
    a = torch.zeros(2, 80, 8)
    with pytest.raises(ValueError, match="one GPU device"):
        mel_distance(a, a, [8, 4])
    with pytest.raises(ValueError, match="same B and M"):
        mel_distance(a, torch.zeros(3, 80, 8), [8, 4])
    with pytest.raises(L.VersbandError):
        MelNet(MEL_HP)(torch.zeros(2, 6400), lengths=[6400, 3200])           # no CPU path, with lengths or without


# ---------------------------------------------------------------------------------------------------------------- the route facts
def test_the_stft_convolution_runs_an_exact_fp32_kernel_at_every_length():
    """THE BIT-FOR-BIT CONTRACT rests on this: Ci = hop, Co = 2 * im_off, k = n_fft / hop, fp32 weights only.  Whatever T_out and B, the
    route is one of the two exact-fp32 kernels, which accumulate in one order (tests/test_gpu_conv_units.py SAME_BITS, tests/test_gpu_kernels.py compare them bit for bit): the DMA-fed
    one when the block count J = T + taps - 1 is a multiple of 4, the register-staged one otherwise.  Never the minimal-filtering kernel
    (no such weights), never a bf16 / split one.  (The plan takes no transposed-output flag; that flag only rules the staged epilogue out.)"""
    lib = L.load()
    co4 = 2 * ((N_FFT // 2 + 1 + 3) // 4 * 4)
    seen = set()
    for B in (1, 6, 8):
        for T in sorted({frames_of(n, False) for n in LENS} | {frames_of(n, True) for n in LENS_CENTER} | {1200, 1500, 1504}):
            J = T + TAPS - 1
            r, tc, tt, se = C.c_int(-1), C.c_int(), C.c_int(), C.c_int()
            rc = lib.vb_conv1d_plan(B, HOP, J, co4, TAPS, 1, 0, 0, 0, 0, T, 0, 1, 0, 0, 0, 1.0, 0.0, 1, 0, 0, 0, 0, C.byref(r), C.byref(tc), C.byref(tt), C.byref(se))
            assert rc == 0, lib.vb_last_error()
            assert r.value == (7 if J % 4 == 0 else 8), (B, T, r.value)           # VB_ROUTE_F32G / VB_ROUTE_F32
            seen.add(r.value)
    assert seen == {7, 8}, "the lengths of the GPU test reach both kernels: rows and clips alone take different routes there"
    assert {(frames_of(n, False) + TAPS - 1) % 4 == 0 for n in LENS} == {True, False}


# ---------------------------------------------------------------------------------------------------------------- the index arithmetic
def _mel_from_frames(fr, fb):
    """ref_cpu.melnet_forward from its unfold on: frames [1, T, n_fft] float32 -> log10-mel [n_mels, T], the same torch operations on the
    same shapes"""
    spec = torch.fft.rfft(fr.double() * torch.hann_window(MEL_HP["win_size"]).double(), dim=-1)
    re, im = spec.real.float(), spec.imag.float()
    mag = torch.sqrt(re.pow(2) + im.pow(2) + 1e-9)
    return torch.log10(torch.clamp(torch.matmul(fb.float(), mag.transpose(1, 2)), min=1e-5))[0]


@pytest.mark.parametrize("center,lens", [(False, LENS), (True, LENS_CENTER)])
def test_two_reflections_at_the_rows_own_end_equal_the_oracle_on_the_clip_alone(center, lens):
    """a row of L_b samples inside a call padded to L: gathering through the restated index and running the oracle's own STFT / mel / log on
    the hop-blocks gives ref_cpu.melnet_forward on the clip alone EXACTLY, the blocks behind J_b are zeros, and no index reaches the padding"""
    Lmax = max(lens)
    fb = torch.from_numpy(mel_filterbank(MEL_HP["audio_sample_rate"], N_FFT, 80, MEL_HP["fmin"], MEL_HP["fmax"]))
    for b, n in enumerate(lens):
        wav = prng.uniform(900 + b, Lmax, -1.3, 1.3).astype(np.float32)
        wav[n:] = np.nan
        idx, Jb = frames_index(Lmax, n, center)
        Tb = frames_of(n, center)
        assert Jb == Tb + TAPS - 1 and (idx[Jb:] == -1).all() and (idx[:Jb] >= 0).all()
        X = np.where(idx >= 0, np.clip(wav[np.maximum(idx, 0)], -1.0, 1.0), 0.0).astype(np.float32)          # [J][hop]
        assert np.isfinite(X).all(), "the NaN padding is never gathered"
        blocks = torch.from_numpy(X[:Jb].reshape(-1))
        got = _mel_from_frames(blocks[None].unfold(-1, N_FFT, HOP), fb)
        ref = ref_cpu.melnet_forward(torch.from_numpy(wav[:n])[None], MEL_HP, fb, center=center)[0]
        assert got.shape == ref.shape == (80, Tb)
        assert torch.equal(got, ref), (n, float((got - ref).abs().max()))
        if n < Lmax:       # ... and with the call's one L in place of L_b the last frames differ: the table is what makes the row right
            wz = np.where(np.isnan(wav), 0.0, wav).astype(np.float32)
            idx_l, _ = frames_index(Lmax, Lmax, center)
            Xl = np.clip(wz[idx_l], -1.0, 1.0).astype(np.float32)
            pl = _mel_from_frames(torch.from_numpy(Xl.reshape(-1))[None].unfold(-1, N_FFT, HOP), fb)[:, :Tb]
            assert not torch.equal(pl[:, -1], ref[:, -1])
