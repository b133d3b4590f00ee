"""HiFi-GAN with row lengths, host side (no GPU): the planner of the vocoder calls, the Python mirror of the library's length checks and
the declaration of the two entry points.  The GPU half is tests/test_gpu_vocoder_lens.py."""
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from versband_amd import _lib as L
from versband_amd import harness
from versband_amd.engine import ConvNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("lens", [[300, 304, 302, 306, 300, 308], [24, 22, 13, 7], [5, 1], [7], [9, 5, 1, 13], [400, 336, 264],
                                  [1, 2, 3, 4, 5, 6, 7, 8, 9]])
def test_plan_groups_partition_the_rows_by_residue(lens):
    calls = harness.plan_vocoder_calls(lens)
    assert sorted(itertools.chain.from_iterable(c["rows"] for c in calls)) == list(range(len(lens))), "the groups partition the rows"
    assert 1 <= len(calls) <= 4
    for c in calls:
        assert len({lens[r] % 4 for r in c["rows"]}) == 1, "members share the residue mod 4"
        assert c["length"] == max(lens[r] for r in c["rows"]), "the padded length is the group's longest member"
        assert c["rows"] == sorted(c["rows"])
        if c["lengths"] is None:
            assert all(lens[r] == c["length"] for r in c["rows"])
        else:
            assert c["lengths"] == [lens[r] for r in c["rows"]] and min(c["lengths"]) < c["length"]
    assert len({lens[c["rows"][0]] % 4 for c in calls}) == len(calls), "one group per residue"
    firsts = [c["rows"][0] for c in calls]
    assert firsts == sorted(firsts), "groups come in the order in which their residues first appear"


def test_plan_equal_lengths_is_one_plain_call_and_even_lengths_make_two_at_most():
    assert harness.plan_vocoder_calls([300] * 5) == [{"rows": [0, 1, 2, 3, 4], "length": 300, "lengths": None}]
    assert harness.plan_vocoder_calls([]) == []
    calls = harness.plan_vocoder_calls([2 * t for t in (150, 152, 151, 153, 150, 154)])
    assert calls == [{"rows": [0, 1, 4, 5], "length": 308, "lengths": [300, 304, 300, 308]}, {"rows": [2, 3], "length": 306, "lengths": [302, 306]}]
    assert harness.plan_vocoder_calls([8, 4, 6, 6]) == [{"rows": [0, 1], "length": 8, "lengths": [8, 4]}, {"rows": [2, 3], "length": 6, "lengths": None}]
    for lens in ([2 * t for t in range(1, 40)], [600, 602]):
        assert len(harness.plan_vocoder_calls(lens)) <= 2
    again = harness.plan_vocoder_calls([24, 22, 13, 7])
    assert again == harness.plan_vocoder_calls([24, 22, 13, 7]) and [c["rows"] for c in again] == [[0], [1], [2], [3]]
    with pytest.raises(ValueError, match="row 1 has length 0"):
        harness.plan_vocoder_calls([4, 0])


# ---------------------------------------------------------------------------------------------------------------- Python checks
def _net(which, in_ch=80, in_tmul=1):
    """a ConvNet that never reaches the library: the checks under test come before the first call into it"""
    net = object.__new__(ConvNet)
    net.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul = which, in_ch, 1, 320, in_tmul
    return net


def test_python_length_checks_use_the_library_wording():
    """lens_plan (versband_amd/csrc/sampler_step.hip's rules: B <= 64, 1 <= len[b] <= T, the row named), stated by the host first - in the
    words DiTEngine.sample_cfg(lengths=) uses"""
    voc, mel = _net(L.NET_VOCODER), torch.zeros(3, 80, 24)
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0 is not in \[1, T = 24\]"), ([24, 12, 25], r"lengths\[2\] = 25 is not in \[1, T = 24\]"),
                       ([24, 12], "lengths"), ([24, 12.5, 3], "lengths")):
        with pytest.raises((ValueError, TypeError), match=text):
            voc.run(mel, lengths=lens)
    with pytest.raises(ValueError, match=r"65 rows \(at most 64\)"):
        voc.run(torch.zeros(65, 80, 24), lengths=[12] * 65)
    from versband_amd.engine import DiTEngine
    for lens in ([24, 0, 12], [24, 12, 25]):           # the same sentence as the sampler's lengths=
        with pytest.raises(ValueError) as sampler:
            DiTEngine._lens_struct(lens, 3, 24)
        with pytest.raises(ValueError) as vocoder:
            voc.run(mel, lengths=lens)
        assert str(sampler.value) == str(vocoder.value)


def test_only_the_vocoder_net_accepts_lengths():
    for which, name in ((L.NET_VAE, "VAE decoder"), (L.NET_VAE_ENCODER, "VAE encoder")):
        with pytest.raises(ValueError, match=name):
            _net(which, in_ch=20).run(torch.zeros(2, 20, 16), lengths=[16, 8])


def test_spec2wav_batch_hands_lengths_to_the_net():
    from versband_amd.model import HifiGAN
    seen = []
    voc = object.__new__(HifiGAN)
    voc.net = lambda: SimpleNamespace(run=lambda mel, **kw: seen.append(kw) or torch.zeros(mel.shape[0], 1, 8))
    assert voc.spec2wav_batch(torch.zeros(2, 80, 4)).shape == (2, 8) and seen == [{}]
    voc.spec2wav_batch(torch.zeros(2, 80, 4), lengths=[4, 2])
    assert seen[1] == {"lengths": [4, 2]}


# ---------------------------------------------------------------------------------------------------------------- header
def test_header_declares_both_entry_points_and_the_binding_knows_them():
    text = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    assert re.search(r"size_t\s+vb_hifigan_lens_workspace_bytes\(vb_ctx\*\s*\w*,\s*int B,\s*int T\);", text)
    assert re.search(r"int\s+vb_hifigan_forward_lens\(vb_ctx\*\s*\w*,\s*const float\*\s*mel,\s*int B,\s*int T,\s*const vb_lens\*\s*lens,\s*float\*\s*wav,"
                     r"\s*void\*\s*ws,\s*void\*\s*stream\);", text)
    assert len(L.PROTOTYPES["vb_hifigan_forward_lens"][1]) == 8 and len(L.PROTOTYPES["vb_hifigan_lens_workspace_bytes"][1]) == 3
    assert "route" in text.lower() and "(mod 4)" in text
