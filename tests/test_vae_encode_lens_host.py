"""VAE encoder with row lengths, host side (no GPU): the planner of the encode calls, the Python mirror of the library's length checks,
the lengths path of the model's encode methods and the declaration of the entry points.  The GPU half is tests/test_gpu_vae_encode_lens.py."""
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
M = harness.ENCODE_ROUTE_MOD


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("lens", [[150, 152, 151, 153, 150, 154], [24, 22, 13, 7, 1], [5, 1], [7], [96, 68, 36, 4], [70, 66, 38, 6, 2],
                                  [1, 2, 3, 4, 5, 6, 7, 8, 9]])
def test_plan_groups_partition_the_rows_by_the_route_rule(lens):
    calls = harness.plan_encode_calls(lens)
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
    firsts = [c["rows"][0] for c in calls]
    assert firsts == sorted(firsts), "groups come in the order in which their residues first appear"


def test_plan_equal_lengths_is_one_plain_call_and_bad_lengths_are_rejected():
    assert M == 4
    assert harness.plan_encode_calls([150] * 5) == [{"rows": [0, 1, 2, 3, 4], "length": 150, "lengths": None}]
    assert harness.plan_encode_calls([]) == []
    assert harness.plan_encode_calls([150, 152, 151, 153, 150, 154]) == [
        {"rows": [0, 4, 5], "length": 154, "lengths": [150, 150, 154]}, {"rows": [1], "length": 152, "lengths": None},
        {"rows": [2], "length": 151, "lengths": None}, {"rows": [3], "length": 153, "lengths": None}]
    assert [c["rows"] for c in harness.plan_encode_calls([600, 624, 644, 668, 688, 708, 732, 752])] == [list(range(8))]
    assert harness.plan_encode_calls([7, 3, 5]) == harness.plan_decode_calls([7, 3, 5])      # one unit, one modulus: encode, sample, decode
    with pytest.raises(ValueError, match="plan_encode_calls: row 1 has length 0"):
        harness.plan_encode_calls([4, 0])


# ---------------------------------------------------------------------------------------------------------------- Python checks
def _net(which, in_ch=80, in_tmul=2):
    """a ConvNet that never reaches the library: the checks under test come before the first call into it"""
    net = object.__new__(ConvNet)
    net.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul = which, in_ch, 40, 1, in_tmul
    return net


def test_encode_lens_states_the_library_rules_with_the_sentences_of_decode_lens():
    enc, mel = _net(L.NET_VAE_ENCODER), torch.zeros(3, 80, 48)                       # T = 24 latent tokens
    dec = _net(L.NET_VAE, in_ch=20, in_tmul=1)
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0 is not in \[1, T = 24\]"), ([24, 12, 25], r"lengths\[2\] = 25 is not in \[1, T = 24\]"),
                       ([24, 12], "lengths has 2 entries for 3 rows"), ([24, 12.5, 3], "lengths must hold integers")):
        with pytest.raises((ValueError, TypeError), match=text) as e:
            enc.encode_lens(mel, lens)
        with pytest.raises((ValueError, TypeError)) as d:
            dec.decode_lens(torch.zeros(3, 20, 24), lens)
        assert str(e.value) == str(d.value) and type(e.value) is type(d.value)
    with pytest.raises(ValueError, match=r"65 rows \(at most 64\)"):
        enc.encode_lens(torch.zeros(65, 80, 48), [12] * 65)


def test_encode_lens_is_the_encoders_alone():
    for which, name, ch, tm in ((L.NET_VAE, "VAE decoder", 20, 1), (L.NET_VOCODER, "vocoder", 80, 1)):
        with pytest.raises(ValueError, match=name) as e:
            _net(which, in_ch=ch, in_tmul=tm).encode_lens(torch.zeros(2, ch, 16), [16, 8])
        assert "encode_lens" in str(e.value)
    # the encoder goes on refusing lengths through the other nets' methods, and now says where they go
    enc = _net(L.NET_VAE_ENCODER)
    for call in (lambda: enc.run(torch.zeros(2, 80, 32), lengths=[16, 8]), lambda: enc.decode_lens(torch.zeros(2, 80, 32), [16, 8]),
                 lambda: enc.vocode_lens(torch.zeros(2, 80, 32), [16, 8])):
        with pytest.raises(ValueError, match="VAE encoder") as e:
            call()
        assert "encode_lens" in str(e.value)


def test_encode_lens_needs_whole_latent_tokens():
    enc = _net(L.NET_VAE_ENCODER)
    with pytest.raises(ValueError, match="47 is not a multiple of 2"):
        enc.encode_lens(torch.zeros(2, 80, 47), [23, 8])
    with pytest.raises(ValueError, match="not a multiple of 4"):
        _net(L.NET_VAE_ENCODER, in_tmul=4).encode_lens(torch.zeros(2, 80, 46), [11, 8])


def test_encode_lens_without_lengths_or_with_full_rows_is_run(monkeypatch):
    enc, seen = _net(L.NET_VAE_ENCODER), []
    monkeypatch.setattr(ConvNet, "run", lambda self, x, lengths=None: seen.append((tuple(x.shape), lengths)) or "plain")
    assert enc.encode_lens(torch.zeros(2, 80, 48), None) == "plain" and enc.encode_lens(torch.zeros(2, 80, 48), [24, 24]) == "plain"
    assert seen == [((2, 80, 48), None)] * 2
    assert ConvNet.LENS_WORKSPACE["vb_vae_encode_lens"] == "vb_vae_encode_lens_workspace_bytes"


# ---------------------------------------------------------------------------------------------------------------- model
def test_encode_first_stage_hands_lengths_to_the_net():
    from versband_amd.model import CFM, AutoencoderKL, DiagonalGaussianDistribution
    seen = []
    net = SimpleNamespace(run=lambda x: seen.append(("run", None)) or torch.zeros(x.shape[0], 40, x.shape[-1] // 2),
                          encode_lens=lambda x, lens: seen.append(("lens", list(lens))) or torch.zeros(x.shape[0], 40, x.shape[-1] // 2))
    fs = SimpleNamespace(enc_net=net, enc_state={"k": 0}, _device=None, _precision="fp32mf")
    fs.encode = lambda x, lengths=None: AutoencoderKL.encode(fs, x, lengths=lengths) if lengths is not None else AutoencoderKL.encode(fs, x)
    m = SimpleNamespace(first_stage_model=fs, _context=lambda: SimpleNamespace(device="cpu"))
    post = CFM.encode_first_stage(m, torch.zeros(2, 80, 8))
    assert isinstance(post, DiagonalGaussianDistribution) and post.mean.shape == (2, 20, 4)
    post = CFM.encode_first_stage(m, torch.zeros(2, 80, 8), lengths=[4, 2])
    assert isinstance(post, DiagonalGaussianDistribution) and post.parameters.shape == (2, 40, 4)
    assert seen == [("run", None), ("lens", [4, 2])]


def test_get_first_stage_encoding_without_lengths_is_the_reference_path():
    from versband_amd.model import CFM
    m = SimpleNamespace(scale_factor=torch.tensor(0.5))
    z = torch.arange(6.0).reshape(1, 2, 3)
    assert torch.equal(CFM.get_first_stage_encoding(m, z), 0.5 * z)
    with pytest.raises(NotImplementedError):
        CFM.get_first_stage_encoding(m, [z])


# ---------------------------------------------------------------------------------------------------------------- header
def test_header_declares_the_entry_points_and_the_binding_knows_them():
    text = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    assert re.search(r"size_t\s+vb_vae_encode_lens_workspace_bytes\(vb_ctx\*\s*\w*,\s*int B,\s*int T\);", text)
    assert re.search(r"int\s+vb_vae_encode_lens\(vb_ctx\*\s*\w*,\s*const float\*\s*mel,\s*int B,\s*int T,\s*const vb_lens\*\s*lens,\s*float\*\s*moments,"
                     r"\s*void\*\s*ws,\s*void\*\s*stream\);", text)
    assert re.search(r"int\s+vb_posterior_lens\(const float\*\s*moments,\s*const float\*\s*noise", text)
    assert L.PROTOTYPES["vb_vae_encode_lens"] == L.PROTOTYPES["vb_vae_decode_lens"]
    assert L.PROTOTYPES["vb_vae_encode_lens_workspace_bytes"] == L.PROTOTYPES["vb_vae_decode_lens_workspace_bytes"]
    assert len(L.PROTOTYPES["vb_posterior_lens"][1]) == 9
    assert "len[b] == T (mod %d)" % M in text.split("vb_vae_decode_lens(vb_ctx")[1], "the encoder's rule is stated beside its entry point"
    lib = L.load()
    assert lib.vb_abi_version() == 3
    for name in ("vb_vae_encode_lens", "vb_vae_encode_lens_workspace_bytes", "vb_posterior_lens"):
        assert hasattr(lib, name)
