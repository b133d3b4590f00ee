"""VAE decoder with row lengths, host side (no GPU): the planner of the decode calls, the Python mirror of the library's length checks,
the decode path of scripts/infer_batched.py::sample_group and the declaration of the entry points.  The GPU half is
tests/test_gpu_vae_lens.py."""
import itertools
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

from versband_amd import _lib as L
from versband_amd import harness
from versband_amd.engine import ConvNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = harness.DECODE_ROUTE_MOD


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("lens", [[150, 152, 151, 153, 150, 154], [24, 22, 13, 7, 1], [5, 1], [7], [96, 68, 36, 4], [70, 66, 38, 6, 2],
                                  [1, 2, 3, 4, 5, 6, 7, 8, 9]])
def test_plan_groups_partition_the_rows_by_the_route_rule(lens):
    calls = harness.plan_decode_calls(lens)
    assert sorted(itertools.chain.from_iterable(c["rows"] for c in calls)) == list(range(len(lens))), "every row once"
    assert 1 <= len(calls) <= M
    for c in calls:
        assert len({lens[r] % M for r in c["rows"]}) == 1, "members share the residue of the route rule"
        assert c["length"] == max(lens[r] for r in c["rows"]), "the padded length is the group's longest member"
        assert c["rows"] == sorted(c["rows"])
        if c["lengths"] is None:
            assert all(lens[r] == c["length"] for r in c["rows"])
        else:
            assert c["lengths"] == [lens[r] for r in c["rows"]] and min(c["lengths"]) < c["length"]
    assert len({lens[c["rows"][0]] % M for c in calls}) == len(calls), "one group per residue"
    firsts = [c["rows"][0] for c in calls]
    assert firsts == sorted(firsts), "groups come in the order in which their residues first appear"


def test_plan_equal_lengths_is_one_plain_call_and_bad_lengths_are_rejected():
    assert M == 4
    assert harness.plan_decode_calls([150] * 5) == [{"rows": [0, 1, 2, 3, 4], "length": 150, "lengths": None}]
    assert harness.plan_decode_calls([]) == []
    calls = harness.plan_decode_calls([150, 152, 151, 153, 150, 154])
    assert calls == [{"rows": [0, 4, 5], "length": 154, "lengths": [150, 150, 154]}, {"rows": [1], "length": 152, "lengths": None},
                     {"rows": [2], "length": 151, "lengths": None}, {"rows": [3], "length": 153, "lengths": None}]
    assert [c["rows"] for c in harness.plan_decode_calls([600, 624, 644, 668, 688, 708, 732, 752])] == [list(range(8))]
    with pytest.raises(ValueError, match="row 1 has length 0"):
        harness.plan_decode_calls([4, 0])
    with pytest.raises(ValueError, match="row 0 has length -3"):
        harness.plan_decode_calls([-3])


# ---------------------------------------------------------------------------------------------------------------- Python checks
def _net(which, in_ch=20, in_tmul=1):
    """a ConvNet that never reaches the library: the checks under test come before the first call into it"""
    net = object.__new__(ConvNet)
    net.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul = which, in_ch, 80, 2, in_tmul
    return net


def test_decode_lens_states_the_library_rules_naming_the_argument():
    dec, z = _net(L.NET_VAE), torch.zeros(3, 20, 24)
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0 is not in \[1, T = 24\]"), ([24, 12, 25], r"lengths\[2\] = 25 is not in \[1, T = 24\]"),
                       ([24, 12], "lengths"), ([24, 12.5, 3], "lengths")):
        with pytest.raises((ValueError, TypeError), match=text):
            dec.decode_lens(z, lens)
    with pytest.raises(ValueError, match=r"65 rows \(at most 64\)"):
        dec.decode_lens(torch.zeros(65, 20, 24), [12] * 65)
    with pytest.raises(ValueError) as voc:
        _net(L.NET_VOCODER, in_ch=80).run(torch.zeros(3, 80, 24), lengths=[24, 0, 12])
    with pytest.raises(ValueError) as vae:
        dec.decode_lens(z, [24, 0, 12])
    assert str(voc.value) == str(vae.value)            # the sentence of the sampler's and the vocoder's lengths=


def test_decode_lens_is_the_decoders_alone_and_run_keeps_refusing_lengths():
    for which, name in ((L.NET_VAE_ENCODER, "VAE encoder"), (L.NET_VOCODER, "vocoder")):
        with pytest.raises(ValueError, match=name):
            _net(which).decode_lens(torch.zeros(2, 20, 16), [16, 8])
    for which, name in ((L.NET_VAE, "VAE decoder"), (L.NET_VAE_ENCODER, "VAE encoder")):
        with pytest.raises(ValueError, match=name):
            _net(which).run(torch.zeros(2, 20, 16), lengths=[16, 8])
    with pytest.raises(ValueError, match="decode_lens"):
        _net(L.NET_VAE).run(torch.zeros(2, 20, 16), lengths=[16, 8])


def test_decode_first_stage_hands_lengths_to_the_net():
    from versband_amd.model import CFM
    seen = []
    net = SimpleNamespace(run=lambda z: seen.append(("run", None)) or torch.zeros(z.shape[0], 80, 2 * z.shape[-1]),
                          decode_lens=lambda z, lens: seen.append(("lens", list(lens))) or torch.zeros(z.shape[0], 80, 2 * z.shape[-1]))
    m = SimpleNamespace(vae_net=lambda: net)
    assert CFM.decode_first_stage(m, torch.zeros(2, 20, 4)).shape == (2, 80, 8)
    CFM.decode_first_stage(m, torch.zeros(2, 20, 4), lengths=[4, 2])
    assert seen == [("run", None), ("lens", [4, 2])]


# ---------------------------------------------------------------------------------------------------------------- CLI decode path
def test_sample_group_decodes_once_per_planned_group(monkeypatch):
    """sample_group with a stub model: six items of 150, 152, 151, 153, 150, 154 tokens in one sampler call with row lengths; the decode
    runs once per group of harness.plan_decode_calls, each padded to its longest row, and every mel comes out at its own length"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import infer_batched as ib
    tokens = [150, 152, 151, 153, 150, 154]
    decodes, vocodes = [], []

    def decode_first_stage(z, lengths=None):
        decodes.append((tuple(z.shape), None if lengths is None else list(lengths)))
        return z[:, :1].repeat_interleave(2, dim=-1).expand(-1, 80, -1).clone()        # mel frame 2t, 2t + 1 = latent token t, channel 0

    def sample_cfg(**kw):
        B, (C, T) = kw["batch_size"], kw["shape"]
        assert kw["lengths"] == tokens
        z = torch.zeros(B, C, T)
        for r in range(B):
            z[r, :, :tokens[r]] = 1.0 + r
            z[r, :, tokens[r]:] = float("nan")          # the sampler's padding is zero in the product; the decode path must not care
        return z, None

    model = SimpleNamespace(first_stage_model=SimpleNamespace(embed_dim=20), decode_first_stage=decode_first_stage)
    sampler = SimpleNamespace(model=model, sample_cfg=sample_cfg)

    def spec2wav_batch(mel, lengths=None):
        vocodes.append((tuple(mel.shape), lengths))
        return torch.zeros(mel.shape[0], mel.shape[-1] * 4)

    monkeypatch.setattr(ib, "_item_conditioning", lambda *a, **k: ({}, {}))
    monkeypatch.setattr(ib, "_cat_conditioning", lambda parts, frames=None: {})
    args = SimpleNamespace(n_samples=1, seed=0, items_per_batch=6, length_slack=8, ddim_steps=2, guidance_interval=None)
    group = [(i, {"acoustic": torch.zeros(80, t * harness.MEL_DOWNSAMPLE)}) for i, t in enumerate(tokens)]
    out = ib.sample_group(args, sampler, SimpleNamespace(spec2wav_batch=spec2wav_batch), group, [3.0], torch.device("cpu"))
    plan = harness.plan_decode_calls(tokens)
    assert decodes == [((len(c["rows"]), 20, c["length"]), c["lengths"]) for c in plan]
    assert len(decodes) == 4 < len(set(tokens)) and decodes[0] == ((3, 20, 154), [150, 150, 154])
    for p, t in enumerate(tokens):
        mel, _ = out[(p, 3.0)][0]
        assert mel.shape == (80, 2 * t) and bool((mel == 1.0 + p).all()), "every mel is its own row, cut to its own length"
    assert sum(shape[0] for shape, _ in vocodes) == len(tokens)


# ---------------------------------------------------------------------------------------------------------------- header
def test_header_declares_both_entry_points_and_the_binding_knows_them():
    text = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    assert re.search(r"size_t\s+vb_vae_decode_lens_workspace_bytes\(vb_ctx\*\s*\w*,\s*int B,\s*int T\);", text)
    assert re.search(r"int\s+vb_vae_decode_lens\(vb_ctx\*\s*\w*,\s*const float\*\s*z,\s*int B,\s*int T,\s*const vb_lens\*\s*lens,\s*float\*\s*mel,"
                     r"\s*void\*\s*ws,\s*void\*\s*stream\);", text)
    assert len(L.PROTOTYPES["vb_vae_decode_lens"][1]) == 8 and len(L.PROTOTYPES["vb_vae_decode_lens_workspace_bytes"][1]) == 3
    assert len(L.PROTOTYPES["vb_gn_stats_lens"][1]) == 9 and len(L.PROTOTYPES["vb_softmax_rows_t_lens"][1]) == 6
    assert L.PROTOTYPES["vb_vae_decode_lens"] == L.PROTOTYPES["vb_hifigan_forward_lens"]
    assert "len[b] == T (mod %d)" % M in text
