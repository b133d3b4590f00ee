"""BigVGAN with row lengths, host side (no GPU): the binding of the new symbols, the Python checks that come before any library call, and
the oracle's statement of why the anti-aliased activation needed a kernel change (the GPU half is tests/test_gpu_bigvgan_lens.py)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as TF

from oracle import ref_cpu
from versband_amd import _lib as L
from versband_amd.engine import ConvNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = C.c_void_p, C.c_int
LENS = C.POINTER(L.Lens)
# the header's parameter lists, by type: pointers (P), ints (I), const vb_lens* (LENS)
SIGNATURES = {
    "vb_bigvgan_lens_workspace_bytes": (C.c_size_t, [P, I, I]),
    "vb_bigvgan_forward_lens": (I, [P, P, I, I, LENS, P, P, P]),
    "vb_bigvgan_chunked_lens_workspace_bytes": (C.c_size_t, [P, I, I, I, I]),
    "vb_bigvgan_forward_chunked_lens": (I, [P, P, I, I, I, I, LENS, P, P, P, P, P]),
    "vb_aa_act": (I, [P, P, P, P, I, I, I, P, I, P, P]),
}


def _header_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "versband_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in the header"
    kinds = []
    for p in m.group(2).split(","):
        p = " ".join(p.split())
        kinds.append(LENS if "vb_lens" in p else (P if "*" in p else I))
    return (C.c_size_t if m.group(1) == "size_t" else I), kinds


@pytest.mark.parametrize("name", list(SIGNATURES))
def test_binding_declares_the_new_symbols_with_the_headers_signatures(name):
    assert L.PROTOTYPES[name] == SIGNATURES[name]
    assert _header_params(name) == SIGNATURES[name]


def test_the_hifigan_twins_have_the_same_shapes():
    assert L.PROTOTYPES["vb_bigvgan_forward_lens"] == L.PROTOTYPES["vb_hifigan_forward_lens"]
    assert L.PROTOTYPES["vb_bigvgan_forward_chunked_lens"] == L.PROTOTYPES["vb_hifigan_forward_chunked_lens"]
    assert L.PROTOTYPES["vb_bigvgan_lens_workspace_bytes"] == L.PROTOTYPES["vb_hifigan_lens_workspace_bytes"]
    assert L.PROTOTYPES["vb_bigvgan_chunked_lens_workspace_bytes"] == L.PROTOTYPES["vb_hifigan_chunked_lens_workspace_bytes"]


# ---------------------------------------------------------------------------------------------------------------- Python checks
def _net(which, in_ch=80, in_tmul=1):
    """a ConvNet that never reaches the library: the checks under test come before the first call into it"""
    net = object.__new__(ConvNet)
    net.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul = which, in_ch, 1, 320, in_tmul
    return net


def test_vocode_lens_rejects_bad_lengths_before_any_library_call():
    net, mel = _net(L.NET_VOCODER), torch.zeros(3, 80, 24)
    for kw in ({}, {"chunk": 8, "halo": 4}):
        for lens, text in (([24, 0, 12], r"lengths\[1\] = 0 is not in \[1, T = 24\]"), ([24, 12, 25], r"lengths\[2\] = 25 is not in \[1, T = 24\]"),
                           ([24, 12], "lengths has 2 entries for 3 rows")):
            with pytest.raises(ValueError, match=text):
                net.vocode_lens(mel, lens, **kw)
        with pytest.raises(ValueError, match="65 rows"):
            net.vocode_lens(torch.zeros(65, 80, 24), [12] * 65, **kw)
    for chunk, halo in ((0, 4), (8, -1)):
        with pytest.raises(ValueError, match=f"chunk = {chunk}, halo = {halo}"):
            net.vocode_lens(mel, [24, 12, 8], chunk=chunk, halo=halo)


def test_vocode_lens_is_the_vocoders_alone():
    for which, name in ((L.NET_VAE, "VAE decoder"), (L.NET_VAE_ENCODER, "VAE encoder")):
        with pytest.raises(ValueError, match=f"the {name} has no vocode_lens"):
            _net(which, in_ch=20).vocode_lens(torch.zeros(2, 20, 16), [16, 8])


def test_no_lengths_and_full_rows_fall_through_to_run_and_run_chunked():
    net, seen = _net(L.NET_VOCODER), []
    net.run = lambda x, **kw: seen.append(("run", kw)) or torch.zeros(x.shape[0], 1, 2)
    net.run_chunked = lambda x, chunk, halo, **kw: seen.append(("chunked", chunk, halo, kw)) or torch.zeros(x.shape[0], 1, 2)
    mel = torch.zeros(2, 80, 40)
    net.vocode_lens(mel, None)
    net.vocode_lens(mel, [40, 40])
    net.vocode_lens(mel, None, chunk=8, halo=4)
    net.vocode_lens(mel, [40, 40], chunk=8)
    assert seen == [("run", {}), ("run", {}), ("chunked", 8, 4, {}), ("chunked", 8, 32, {})]


def test_vocode_batch_hands_lengths_and_chunk_to_vocode_lens():
    from versband_amd.model import VocoderBigVGAN
    seen = []
    voc = object.__new__(VocoderBigVGAN)
    voc.net = lambda: SimpleNamespace(vocode_lens=lambda mel, lengths, **kw: seen.append((lengths, kw)) or torch.zeros(mel.shape[0], 1, 8))
    assert voc.vocode_batch(torch.zeros(2, 80, 4)).shape == (2, 8)
    voc.vocode_batch(torch.zeros(2, 80, 4), lengths=[4, 2], chunk=16, halo=4)
    assert seen == [(None, {"chunk": None, "halo": 32}), ([4, 2], {"chunk": 16, "halo": 4})]


# ---------------------------------------------------------------------------------------------------------------- why a kernel
class _FiltersInTheRowsDtype:
    """ref_cpu builds the anti-aliasing filter in fp32; the float64 oracle casts it to the row's dtype"""

    def __getattr__(self, name):
        return getattr(TF, name)

    def conv1d(self, x, w, *args, **kw):
        return TF.conv1d(x, w.to(x.dtype), *args, **kw)

    def conv_transpose1d(self, x, w, *args, **kw):
        return TF.conv_transpose1d(x, w.to(x.dtype), *args, **kw)


@pytest.mark.parametrize("n", [1, 3, 6, 40, 257])
def test_a_zero_tail_reaches_five_samples_into_the_row(n, monkeypatch):
    """The activation replicate-pads at the row end in both filters.  On a zero-padded row the samples next to the end see zeros where
    the clip alone sees its last sample again, so they differ; further in the two are the same.  Measured here, not derived: the
    difference reaches min(n, 5) samples from the row's end (output t reads the up-sampled signal up to 2 t + 6, and that reads x up to
    t + 5) - few samples, but enough that the vocoder's zero-tail machinery could not carry this op, and its kernel now takes the row's
    own end instead (net_glue.hip: aa_act_kernel)."""
    monkeypatch.setattr(ref_cpu, "F", _FiltersInTheRowsDtype())
    g = torch.Generator().manual_seed(7)
    T = n + 40
    x = torch.randn(1, 3, T, dtype=torch.float64, generator=g)
    x[..., n:] = 0
    alpha, beta = torch.tensor([0.6, 1.0, 1.7], dtype=torch.float64), torch.tensor([1.3, 0.8, 0.5], dtype=torch.float64)
    row = ref_cpu.aa_activation(x, alpha, beta, False)[..., :n]
    clip = ref_cpu.aa_activation(x[..., :n].contiguous(), alpha, beta, False)
    d = (row - clip).abs().amax(dim=(0, 1))
    differs = (d > 1e-9).nonzero().flatten()
    reach = n - int(differs.min())
    print(f"n = {n}: the zero tail changes the last {reach} samples, by up to {float(d.max()):.3e}")
    assert reach == min(n, 5)
    assert float(d[:n - reach].max() if n > reach else 0.0) <= 1e-12
    assert float(d[n - reach:].min()) > 1e-6          # every one of them, and by far more than roundoff
