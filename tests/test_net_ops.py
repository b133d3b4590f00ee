"""The conv-net op lists name their weight format (vb_net_op.wfmt, include/versband_hip.h): every builder at every precision emits
ops that pass vb_net_load's rules (CPU, the builders run on device="cpu" with ConvNet stubbed out), and the library refuses
malformed ops at load time (GPU: vb_net_load needs a context)."""
import collections

import pytest
import torch

from versband_amd import _lib as L
from versband_amd import engine, synth

VB_E_INVALID = -1
WEIGHT_FIELDS = ("w", "w_x3", "w_mf", "w2")
# the (kind, wfmt) table of include/versband_hip.h: the weight fields each allowed pair reads
READS = {
    (L.OP_CONV, L.WFMT_F32): {"w"},
    (L.OP_CONV, L.WFMT_X3): {"w_x3", "w"},
    (L.OP_CONV, L.WFMT_MF): {"w_mf", "w"},
    (L.OP_CONV, L.WFMT_BUF_F32): {"w_buf"},
    (L.OP_CONV, L.WFMT_BUF_X3): {"w_buf"},
    (L.OP_RESPAIR, L.WFMT_F32): {"w", "w2"},
    (L.OP_RESPAIR, L.WFMT_X3): {"w_x3", "w2"},
    (L.OP_RESPAIR, L.WFMT_MF): {"w_mf", "w2"},
    (L.OP_AA_ACT, L.WFMT_NONE): {"w"},
    **{(k, L.WFMT_NONE): set() for k in (L.OP_GN_STATS, L.OP_SOFTMAX_T, L.OP_SPLIT_PLANES, L.OP_GN_APPLY, L.OP_XT_PLANES)},
}
# the weight formats each builder precision may emit
FORMATS = {"split": {L.WFMT_NONE, L.WFMT_X3, L.WFMT_BUF_X3}, "fp32": {L.WFMT_NONE, L.WFMT_F32, L.WFMT_BUF_F32},
           "fp32mf": {L.WFMT_NONE, L.WFMT_F32, L.WFMT_MF, L.WFMT_BUF_F32}}
ENV_SWITCHES = ("VB_FP32_PAIRS", "VB_MF_PAIRS_OFF", "VB_LRELU_IN_WINDOW", "VB_FP32_NO_PREPASS")


def load_rule_violation(o, tmul):
    """vb_net_load's per-op checks (convnet.hip); None when the op passes them"""
    reads = READS.get((o.kind, o.wfmt))
    if reads is None:
        return "unknown (kind, wfmt) pair"
    for f in WEIGHT_FIELDS + ("w_buf",):
        is_set = (o.w_buf != -1) if f == "w_buf" else bool(getattr(o, f))
        if is_set != (f in reads):
            return f"{f} {'set but not read' if is_set else 'missing'}"
    if o.wfmt == L.WFMT_X3 and o.ci_pad != (o.Ci + 31) // 32 * 32:
        return f"ci_pad {o.ci_pad} for Ci {o.Ci}"
    if o.wfmt == L.WFMT_MF and ((o.w_mf or 0) % 16 or (o.w2 or 0) % 16):
        return "minimal-filtering weights not 16-byte aligned"
    if o.kind == L.OP_RESPAIR and (not o.bias or not o.bias2 or o.Ci != o.Co or tmul(o.x) != tmul(o.out)):
        return "malformed respair"
    return None


class _Captured:
    """stands in for ConvNet: keeps the builder instead of loading it into a context"""

    def __init__(self, ctx, which, nb, in_ch, out_ch, out_tmul, in_tmul=1):
        self.nb, self.out_tmul, self.in_tmul = nb, out_tmul, in_tmul


def _build(name, precision, monkeypatch):
    monkeypatch.setattr(engine, "ConvNet", _Captured)
    ctx = type("CpuCtx", (), {"device": torch.device("cpu")})()
    vcfg = synth.VAEConfig()
    if name == "vae_decoder":
        return engine.build_vae_decoder(ctx, synth.make_state_dict(synth.vae_decoder_shapes(vcfg), 11), 0.8, precision=precision)
    if name == "vae_encoder":
        return engine.build_vae_encoder(ctx, synth.make_state_dict(synth.vae_encoder_shapes(vcfg), 12), precision=precision)
    if name == "hifigan":
        hcfg = synth.HifiGanConfig()
        return engine.build_hifigan(ctx, synth.make_state_dict(synth.hifigan_shapes(hcfg), 13), hcfg.as_hparams(), precision=precision)
    bcfg = synth.BigVGANConfig()
    return engine.build_bigvgan(ctx, synth.make_state_dict(synth.bigvgan_shapes(bcfg), 14), bcfg.as_hparams(), precision=precision)


# HiFi-GAN of the synthetic default configuration, (kind, wfmt) -> ops: 18 fused pairs in split / fp32; in fp32mf the nine
# 32-channel pairs run on the minimal-filtering pair kernel and the 64-channel pairs as two minimal-filtering convolutions
HIFIGAN_COUNTS = {
    "split": {(L.OP_CONV, L.WFMT_X3): 42, (L.OP_RESPAIR, L.WFMT_X3): 18},
    "fp32": {(L.OP_CONV, L.WFMT_F32): 42, (L.OP_RESPAIR, L.WFMT_F32): 18},
    "fp32mf": {(L.OP_CONV, L.WFMT_F32): 5, (L.OP_CONV, L.WFMT_MF): 55, (L.OP_RESPAIR, L.WFMT_MF): 9},
}


@pytest.mark.parametrize("precision", ["split", "fp32", "fp32mf"])
@pytest.mark.parametrize("name", ["vae_decoder", "vae_encoder", "hifigan", "bigvgan"])
def test_every_op_names_its_weight_format(name, precision, monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    net = _build(name, precision, monkeypatch)
    nb = net.nb
    assert nb.precision == precision

    def tmul(id_):
        return {L.BUF_INPUT: net.in_tmul, L.BUF_OUTPUT: net.out_tmul}.get(id_) or nb.bufs[id_][1]

    counts = collections.Counter()
    for i, o in enumerate(nb.ops):
        assert o.wfmt in FORMATS[precision], (i, o.kind, o.wfmt)
        assert (o.wfmt == L.WFMT_NONE) == (o.kind not in (L.OP_CONV, L.OP_RESPAIR)), (i, o.kind, o.wfmt)
        err = load_rule_violation(o, tmul)
        assert err is None, f"op {i} (kind {o.kind}, wfmt {o.wfmt}): {err}"
        counts[(o.kind, o.wfmt)] += 1
    if precision == "fp32mf":
        assert counts[(L.OP_CONV, L.WFMT_MF)] > 0
    if name == "hifigan":
        assert {k: v for k, v in counts.items() if k[0] in (L.OP_CONV, L.OP_RESPAIR)} == HIFIGAN_COUNTS[precision]
        assert len(nb.ops) == (69 if precision == "fp32mf" else 60)
        assert all(o.Ci == 32 for o in nb.ops if o.kind == L.OP_RESPAIR and o.wfmt == L.WFMT_MF)


@pytest.mark.gpu
def test_net_load_refuses_malformed_ops():
    """vb_net_load checks every op once, before anything runs: an unknown format, a pointer the format reads that is missing, one it
    does not read that is set, and a respair whose input and output differ in length are refused with VB_E_INVALID and the op's index"""
    from versband_amd.engine import Context
    ctx = Context("cuda:0")
    lib = ctx.lib
    w = torch.zeros(4096, device=ctx.device)
    p = w.data_ptr()
    bufs = (L.BufDesc * 2)(L.BufDesc(32, 1, 0), L.BufDesc(32, 2, 0))

    def conv(**kw):
        f = dict(kind=L.OP_CONV, x=L.BUF_INPUT, out=0, res=-1, stats=-1, w_buf=-1, Ci=32, Co=32, ksize=3, dil=1, pad=1, alpha=1.0,
                 acc_scale=1.0, wfmt=L.WFMT_F32, w=p)
        f.update(kw)
        return L.NetOp(**f)

    def pair(**kw):
        f = dict(kind=L.OP_RESPAIR, x=0, out=L.BUF_OUTPUT, res=-1, stats=-1, w_buf=-1, Ci=32, Co=32, ksize=3, dil=1, alpha=1.0,
                 in_slope=0.1, wfmt=L.WFMT_F32, w=p, w2=p, bias=p, bias2=p)
        f.update(kw)
        return L.NetOp(**f)

    def load(op):
        ops = (L.NetOp * 2)(conv(), op)
        return lib.vb_net_load(ctx.handle, L.NET_VOCODER, ops, 2, bufs, 2, 32, 32, 1, 1)

    assert load(pair()) == 0
    assert load(conv(wfmt=L.WFMT_MF, w_mf=p)) == 0
    assert load(pair(wfmt=L.WFMT_MF, w=None, w_mf=p)) == 0
    cases = {
        "unknown format": conv(wfmt=17),
        "MF conv without its minimal-filtering weights": conv(wfmt=L.WFMT_MF),
        "respair without its second weights": pair(w2=None),
        "stray pointer in a slot the format does not read": conv(w_x3=p),
        "fp32 pair carrying minimal-filtering weights": pair(w_mf=p),
        "respair of unequal lengths": pair(out=1),
    }
    for what, op in cases.items():
        assert load(op) == VB_E_INVALID, what
        msg = lib.vb_last_error().decode()
        assert "op 1" in msg, (what, msg)
