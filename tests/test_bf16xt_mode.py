"""The conv nets' "bf16xt" precision, host side (CPU; the GPU half is tests/test_gpu_bf16xt.py): the arithmetic of "bf16" (every product
RN_bf16(weight) * RN_bf16(activated input), fp32 accumulation) on the SHAPE of the split op list - every wide layer's input goes through a
one-plane VB_OP_XT_PLANES (wfmt = VB_WFMT_BF16, a buffer of square = 4) and the BF16 convolution reads that plane by DMA (x_planes = 1).
"bf16" itself keeps its op list; no default moves; vb_abi_version() stays 3 and vb_conv1d_bf16_xt is how a host detects the feature."""
import collections
import os

import pytest

from tests.test_bf16_mode import READS_BF16, _check_bf16_program
from tests.test_net_ops import _build
from versband_amd import _lib as L
from versband_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("vae_decoder", "vae_encoder", "hifigan", "bigvgan")
PLANE_BUF_SPLIT, PLANE_BUF_ONE = 3, 4       # vb_buf_desc.square of a two-plane / a one-plane transposed buffer


@pytest.mark.parametrize("name", NETS)
def test_bf16xt_program_is_the_split_program_in_one_plane(name, monkeypatch):
    xt = _build(name, "bf16xt", monkeypatch).nb
    split = _build(name, "split", monkeypatch).nb
    assert xt.precision == "bf16xt" and len(xt.ops) == len(split.ops)
    for i, (o, s) in enumerate(zip(xt.ops, split.ops)):
        assert o.kind == s.kind, (i, o.kind, s.kind)
        assert (o.Ci, o.Co, o.ksize, o.dil, o.x_planes) == (s.Ci, s.Co, s.ksize, s.dil, s.x_planes), i
        if s.wfmt == L.WFMT_X3:
            assert o.wfmt == L.WFMT_BF16, (i, o.wfmt)
        elif s.kind == L.OP_XT_PLANES:
            assert s.wfmt == L.WFMT_NONE and split.bufs[s.out][2] == PLANE_BUF_SPLIT
            assert o.wfmt == L.WFMT_BF16 and xt.bufs[o.out][2] == PLANE_BUF_ONE, (i, o.wfmt, xt.bufs[o.out])
            assert (o.in_act, o.upsample2, o.stats >= 0) == (s.in_act, s.upsample2, s.stats >= 0), i
        else:
            assert o.wfmt == s.wfmt, (i, o.wfmt, s.wfmt)            # BUF_X3 (the attention's per-clip products) and NONE stay
        if o.kind == L.OP_CONV and o.x_planes:
            assert o.wfmt == L.WFMT_BF16 and xt.bufs[o.x][2] == PLANE_BUF_ONE and o.Co > 1 and o.in_act == L.ACT_NONE, i
    assert not any(b[2] == PLANE_BUF_SPLIT for b in xt.bufs)
    # the fused narrow vocoder pairs stay RESPAIR BF16, exactly those of "bf16"
    pairs = [(o.Ci, o.ksize, o.dil) for o in xt.ops if o.kind == L.OP_RESPAIR]
    assert all(o.wfmt == L.WFMT_BF16 for o in xt.ops if o.kind == L.OP_RESPAIR)
    assert pairs == [(o.Ci, o.ksize, o.dil) for o in _build(name, "bf16", monkeypatch).nb.ops if o.kind == L.OP_RESPAIR]


def test_vae_decoder_bf16xt_has_planes_ops(monkeypatch):
    nb = _build("vae_decoder", "bf16xt", monkeypatch).nb
    planes = [o for o in nb.ops if o.kind == L.OP_XT_PLANES]
    readers = [o for o in nb.ops if o.kind == L.OP_CONV and o.x_planes]
    assert len(planes) >= 1 and len(readers) >= len(planes)         # (the attention block's q / k / v share one planes buffer)
    assert all(o.wfmt == L.WFMT_BF16 for o in planes + readers)


@pytest.mark.parametrize("name", NETS)
def test_bf16xt_reads_the_bf16_rows_of_the_format_table(name, monkeypatch):
    """static-weight ops read w_x3 (+ w2 for a pair), and the fp32 copy w exactly at one output channel"""
    nb = _build(name, "bf16xt", monkeypatch).nb
    seen = collections.Counter()
    for i, o in enumerate(nb.ops):
        if o.kind not in (L.OP_CONV, L.OP_RESPAIR):
            assert not any(getattr(o, f) for f in ("w_x3", "w_mf", "w2")), i
            continue
        if o.w_buf != -1:
            assert o.wfmt == L.WFMT_BUF_X3 and not any(getattr(o, f) for f in ("w", "w_x3", "w_mf", "w2")), i
            continue
        assert o.wfmt == L.WFMT_BF16, (i, o.wfmt)
        reads = READS_BF16[(o.kind, o.kind == L.OP_CONV and o.Co == 1)]
        for f in ("w", "w_x3", "w_mf", "w2"):
            assert bool(getattr(o, f)) == (f in reads), f"op {i}: {f}"
        assert o.ci_pad == (o.Ci + 31) // 32 * 32
        seen[o.kind] += 1
    assert seen[L.OP_CONV] > 0
    assert sum(1 for o in nb.ops if o.kind == L.OP_CONV and o.w) == sum(1 for o in nb.ops if o.kind == L.OP_CONV and o.w_buf == -1 and o.Co == 1)


@pytest.mark.parametrize("name", NETS)
def test_the_bf16_program_is_unchanged(name, monkeypatch):
    counts = _check_bf16_program(_build(name, "bf16", monkeypatch).nb)          # (no XT_PLANES, no x_planes: asserted inside)
    assert counts[(L.OP_CONV, L.WFMT_BF16)] > 0
    if name == "hifigan":
        assert counts == {(L.OP_CONV, L.WFMT_BF16): 42, (L.OP_RESPAIR, L.WFMT_BF16): 18}


def test_models_and_cli_accept_bf16xt(monkeypatch, tmp_path):
    from versband_amd import model
    hcfg = synth.HifiGanConfig()
    voc = model.HifiGAN.from_state(hcfg.as_hparams(), {}, device="cpu", precision="bf16xt")
    assert voc.precision == "bf16xt"
    for cls, kw in ((model.HifiGAN, dict(vocoder_ckpt=str(tmp_path))), (model.VocoderBigVGAN, dict(ckpt_vocoder=str(tmp_path)))):
        with pytest.raises(AssertionError):
            cls(precision="bf17", **kw)
        with pytest.raises(Exception) as e:            # "bf16xt" passes the precision check and fails later, on the empty checkpoint directory
            cls(precision="bf16xt", **kw)
        assert not isinstance(e.value, AssertionError), e.value
    cfg = model.load_config(os.path.join(ROOT, "configs", "vocal2music.yaml"))
    m = model.instantiate_from_config(cfg.model)
    assert m.vocoder_precision == "fp32mf" and m.first_stage_model._precision == "fp32mf"         # defaults do not move
    cfg.model.params["vocoder_precision"] = "bf16xt"
    m = model.instantiate_from_config(cfg.model)
    assert isinstance(m, model.CFM) and m.vocoder_precision == "bf16xt" and m.first_stage_model._precision == "bf16xt"
    cfg.model.params["vocoder_precision"] = "bf17"
    with pytest.raises(AssertionError):
        model.instantiate_from_config(cfg.model)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "scripts"))
    import infer_batched
    args = infer_batched.parse_args(["--synthetic", "1", "--vocoder_precision", "bf16xt"])
    assert args.vocoder_precision == "bf16xt" and args.precision == "bf16"
    assert infer_batched.parse_args(["--synthetic", "1"]).vocoder_precision == "fp32mf"
    with pytest.raises(SystemExit):
        infer_batched.parse_args(["--synthetic", "1", "--vocoder_precision", "bf17"])


def test_abi_stays_3_and_exports_the_unit_entry_point():
    lib = L.load()
    assert lib.vb_abi_version() == 3
    assert hasattr(lib, "vb_conv1d_bf16_xt") and hasattr(lib, "vb_conv1d_bf16_xt_scratch_bytes")
    # the scratch is one bf16 plane of B x (T_eff + 448) rows x Ci channels
    assert lib.vb_conv1d_bf16_xt_scratch_bytes(2, 64, 100, 0) == 2 * (100 + 448) * 64 * 2
    assert lib.vb_conv1d_bf16_xt_scratch_bytes(2, 64, 24, 1) == 2 * (48 + 448) * 64 * 2
