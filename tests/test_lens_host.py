"""Host side of row lengths (vb_lens): the declarations and their ctypes mirror, the grouping rule of scripts/infer_batched.py
--length_slack, the validation in DiTEngine, and the neighbouring argument helpers left as they were.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from versband_amd import _lib as L
from versband_amd import harness
from versband_amd import model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lens_entry_points_are_declared_bound_and_additive():
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("vb_dit_precompute_cond_lens", "vb_dit_forward_lens", "vb_sample_cfg_lens", "vb_attention_lens"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in L.PROTOTYPES, name
    blk = re.search(r"typedef struct \{([^}]*)\} vb_lens;", code).group(1)
    assert re.findall(r"const int32_t\*\s+([a-z0-9_]+)\s*;", blk) == [f[0] for f in L.Lens._fields_] == ["len"]
    assert L.C.sizeof(L.Lens) == L.C.sizeof(L.c_void_p) and L.Lens._fields_[0][1] == L.C.POINTER(L.C.c_int32)
    # every _lens form is its plain form plus ONE pointer, in the place the header gives it
    P = L.PROTOTYPES
    sched, lens = P["vb_sample_cfg_sched"][1], P["vb_sample_cfg_lens"][1]
    assert len(lens) == len(sched) + 1 and lens[:11] == sched[:11] and lens[11] == L.C.POINTER(L.Lens) and lens[12:] == sched[11:]
    pre, prel = P["vb_dit_precompute_cond"][1], P["vb_dit_precompute_cond_lens"][1]
    assert prel[:9] == pre[:9] and prel[9] == L.C.POINTER(L.Lens) and prel[10:] == pre[9:]
    fwd, fwdl = P["vb_dit_forward"][1], P["vb_dit_forward_lens"][1]
    assert fwdl[:9] == fwd[:9] and fwdl[9] == L.C.POINTER(L.Lens) and fwdl[10:] == fwd[9:]
    att, attl = P["vb_attention"][1], P["vb_attention_lens"][1]
    assert attl[:14] == att[:14] and attl[14] == L.c_void_p and attl[15:] == att[14:]
    for name, n_args in (("vb_sample_cfg_lens", 20), ("vb_dit_precompute_cond_lens", 13), ("vb_dit_forward_lens", 14), ("vb_attention_lens", 17)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code).group(1)
        assert len(decl.split(",")) == n_args == len(P[name][1]), name
    lib = L.load()
    assert all(hasattr(lib, n) for n in ("vb_dit_precompute_cond_lens", "vb_dit_forward_lens", "vb_sample_cfg_lens", "vb_attention_lens"))
    assert lib.vb_abi_version() == 3
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_lens;", src, flags=re.S).group(1)
    for needle in ("the call on that clip alone", "never read into a valid token", "finite", "T_mel == 2 T", "VB_E_INVALID", "B > 64", "VALUES",
                   "len[b % B]"):
        assert needle in doc, needle


# ---- the grouping rule ------------------------------------------------------------------------------------------------
LENGTHS = [200, 200, 168, 132, 132, 400, 396, 200, 75, 75, 75, 75, 75]


@pytest.mark.parametrize("ipb", [1, 2, 3, 4, 8])
def test_slack_zero_reproduces_the_present_groups(ipb):
    want = list(harness.stream_groups(range(len(LENGTHS)), LENGTHS.__getitem__, ipb))
    assert list(harness.stream_length_groups(range(len(LENGTHS)), LENGTHS.__getitem__, ipb)) == want
    assert list(harness.stream_length_groups(iter(range(len(LENGTHS))), LENGTHS.__getitem__, ipb, 0)) == want
    for scales in ([3.0], [1.0, 3.0, 4.5]):
        n = 2
        assert harness.plan_row_batches(LENGTHS, scales, n, ipb, length_slack=0) == harness.plan_row_batches(LENGTHS, scales, n, ipb)
        assert all("row_lengths" not in c for c in harness.plan_row_batches(LENGTHS, scales, n, ipb))


def test_slack_groups_hold_the_cap_end_at_a_jump_and_keep_the_order():
    groups = list(harness.stream_length_groups(range(len(LENGTHS)), LENGTHS.__getitem__, 4, 80))
    assert groups == [[0, 1, 2, 3], [4], [5, 6], [7], [8, 9, 10, 11], [12]]
    #        200 200 168 132 | 132 (the cap) | 400 396 (a jump of 268 before, 196 after) | 200 | 75 x 4 (the cap) | 75
    assert [i for g in groups for i in g] == list(range(len(LENGTHS))), "order is preserved, nothing is dropped"
    for g in groups:
        ls = [LENGTHS[i] for i in g]
        assert len(g) <= 4 and max(ls) - min(ls) <= 80
    # the slack bounds the longest against EVERY member, not against the neighbour: 100, 140, 180 drift apart by 80 > 50
    assert list(harness.stream_length_groups([0, 1, 2], [100, 140, 180].__getitem__, 3, 50)) == [[0, 1], [2]]
    assert list(harness.stream_length_groups([0, 1, 2], [180, 140, 100].__getitem__, 3, 50)) == [[0, 1], [2]]
    assert list(harness.stream_length_groups([0, 1, 2], [140, 180, 100].__getitem__, 3, 80)) == [[0, 1, 2]]
    assert list(harness.stream_length_groups([], LENGTHS.__getitem__, 3, 80)) == []
    with pytest.raises(ValueError, match="length_slack"):
        list(harness.stream_length_groups([0], LENGTHS.__getitem__, 3, -1))


def test_plan_carries_the_row_lengths_of_a_mixed_group():
    calls = harness.plan_row_batches([200, 168, 132, 132], [1.0, 3.0, 4.5], 2, 3, indices=[4, 9, 2, 7], length_slack=80)
    assert [(c["n_branch"], c["items"], c["length"]) for c in calls] == [(2, [0, 1, 2], 200), (1, [0, 1, 2], 200), (2, [3], 132), (1, [3], 132)]
    assert calls[0]["row_lengths"] == [200] * 4 + [168] * 4 + [132] * 4 and calls[1]["row_lengths"] == [200, 200, 168, 168, 132, 132]
    assert "row_lengths" not in calls[2] and "row_lengths" not in calls[3]
    assert calls[0]["clip_ids"] == [8, 9, 8, 9, 18, 19, 18, 19, 4, 5, 4, 5], "the noise key of a row does not depend on its group"
    with pytest.raises(ValueError, match="rows per sampler call"):
        harness.plan_row_batches([200] * 40, [3.0], 1, 33, length_slack=80)


def test_cli_parses_length_slack(monkeypatch):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import infer_batched
    base = ["--synthetic", "2"]
    assert infer_batched.parse_args(base).length_slack == 0
    assert infer_batched.parse_args(base + ["--length_slack", "80", "--items_per_batch", "3"]).length_slack == 80
    with pytest.raises(SystemExit):
        infer_batched.parse_args(base + ["--length_slack", "-1"])


# ---- the Python argument checks ----------------------------------------------------------------------------------------
def test_engine_validates_and_lays_out_the_lengths():
    from versband_amd.engine import DiTEngine
    ls, held, lens = DiTEngine._lens_struct([200, 128, 65, 40], 4, 200)
    assert [ls.len[b] for b in range(4)] == [200, 128, 65, 40] and held is not None and lens == (200, 128, 65, 40)
    ls, _, lens = DiTEngine._lens_struct(torch.tensor([5, 1]), 2, 5)
    assert [ls.len[b] for b in range(2)] == [5, 1] and lens == (5, 1)
    assert DiTEngine._lens_struct([7, np.int64(7)], 2, 7) == (None, None, None), "all rows full is the plain call"
    assert DiTEngine._lens_struct(None, 2, 7) == (None, None, None)
    assert DiTEngine._lens_struct([7, 7], 2, 7, windows=[0, 4]) == (None, None, None), "full rows go with windows"
    for bad, exc, pat in (([200, 0, 65, 40], ValueError, r"lengths\[1\] = 0"), ([200, 128, 201, 40], ValueError, r"lengths\[2\] = 201"),
                          ([200, 128, 65], ValueError, "3 entries for 4 rows"), ([200, 128, 65, -1], ValueError, r"lengths\[3\]"),
                          ([200, 128.0, 65, 40], TypeError, "integers"), ([True, 1, 1, 1], TypeError, "integers"), (7, TypeError, "sequence")):
        with pytest.raises(exc, match=pat):
            DiTEngine._lens_struct(bad, 4, 200)
    with pytest.raises(ValueError, match="windows"):
        DiTEngine._lens_struct([200, 128, 65, 40], 4, 200, windows=[0, 150])
    assert DiTEngine._lens_struct([200, 128, 65, 40], 4, 200, windows=[0])[2] == (200, 128, 65, 40), "one window is the plain call"
    with pytest.raises(ValueError, match="at most 64"):
        DiTEngine._lens_struct([3] * 65, 65, 4)
    with pytest.raises(ValueError, match="2 \\* T = 400"):
        DiTEngine._lens_struct([200, 128, 65, 40], 4, 200, T_mel=402)
    DiTEngine._lens_struct([200] * 4, 4, 200, T_mel=402)       # without short rows the +-2 tolerance stays
    # the conditioning handle remembers its lengths: sampling it with others is refused, in both directions
    made = {"lengths": (200, 128, 65, 40)}
    assert DiTEngine._lens_struct([200, 128, 65, 40], 4, 200, cond=made)[2] == made["lengths"]
    for other in (None, [200, 128, 65, 41], [200] * 4):
        with pytest.raises(ValueError, match="conditioning was made with"):
            DiTEngine._lens_struct(other, 4, 200, cond=made)
    with pytest.raises(ValueError, match="conditioning was made with"):
        DiTEngine._lens_struct([200, 128, 65, 40], 4, 200, cond={"B": 4})
    assert DiTEngine._lens_struct([200] * 4, 4, 200, cond={"B": 4}) == (None, None, None)


def test_neighbouring_argument_helpers_are_unchanged_beside_lengths():
    """guidance_arg and keep_block take no lengths and give what they gave: the blocks compose in the library, token by token"""
    assert vm.guidance_arg([0.0, 1.0, 0.5], None, 4) == [0.0, 1.0, 0.5] and vm.guidance_arg(None, None, 4) is None
    assert vm.guidance_arg(None, (0.0, 1.0), 4) is None
    shape = (2, 20, 12)
    g = torch.Generator().manual_seed(3)
    ref, x0, mask = torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.zeros(2, 12)
    mask[0, 3:9] = 1.0
    blk = vm.keep_block(ref, mask, None, x0, None, shape, 4, 1e-4)
    assert torch.equal(blk[0], ref) and torch.equal(blk[1], x0) and torch.equal(blk[2], mask) and blk[3] == vm.euler_times(4) and blk[4] == 1e-4
    import inspect
    assert "lengths" not in inspect.signature(vm.guidance_arg).parameters and "lengths" not in inspect.signature(vm.keep_block).parameters
    sig = inspect.signature(vm.CFMSampler.sample_cfg).parameters
    assert sig["lengths"].kind is inspect.Parameter.KEYWORD_ONLY and sig["lengths"].default is None
