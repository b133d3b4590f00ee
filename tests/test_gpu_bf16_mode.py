"""The conv nets' single-pass bf16 precision on the GPU: vb_conv1d_bf16 / vb_respair_bf16 against the mode's definition (float64 sums of
exact products of bf16-rounded operands), the five net fixtures in bf16 mode against the CPU restatement and the reference goldens
(bounds from tests/test_bf16_mode.py: (b) x 4 and (a) x 1.25), determinism, and vb_net_load's refusals for the BF16 format."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import describe, rel_l2
from tests.test_bf16_mode import bf16_round, fixture_case, pair_restatement, restatement, FIXTURES
from tests.test_gpu_kernels import CONV_CASES, dev, rnd, sync
from versband_amd import _lib as L
from versband_amd import pack

pytestmark = pytest.mark.gpu
VB_E_INVALID = -1
TOL = 2e-6          # the project's bound for fp32-accumulating kernels (tests/test_gpu_kernels.py): only the accumulation order differs


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    return Context("cuda:0")


def conv_bf16(lib, x, wpacked, bias, B, Ci, T_in, Co, k, dil, pad, T_out, tr=(1, 0, 0), upsample2=0, in_stride=1, in_phase=0, act=0, slope=0.1,
              gn=None, res=None, alpha=1.0, beta=0.0, out=None):
    plane, cip = pack.pack_conv_bf16(wpacked)
    if out is None:
        out = torch.full((B, Co, T_out), float("nan"), device="cuda")
    gm, gr, gg, gb, groups = gn if gn is not None else (None, None, None, None, 0)
    L.check(lib.vb_conv1d_bf16(L.ptr(dev(x)), L.ptr(dev(plane)), cip, L.ptr(dev(bias)) if bias is not None else None, B, Ci, T_in, Co, k, dil,
                               pad, tr[0], tr[1], tr[2], T_out, upsample2, in_stride, in_phase, act, slope,
                               L.ptr(dev(gm)) if gn else None, L.ptr(dev(gr)) if gn else None, L.ptr(dev(gg)) if gn else None,
                               L.ptr(dev(gb)) if gn else None, groups, L.ptr(dev(res)) if res is not None else None, alpha, beta, L.ptr(out),
                               L.stream_ptr()), "conv1d_bf16")
    sync()
    return out


def r64(t):
    """the operand the kernel multiplies: the fp32 value rounded to bf16, as float64"""
    return bf16_round(t.float()).double()


RAGGED = (2, 48, 200, 40, 7, 3, 1, True)      # ragged in every tile dimension, Ci below the pad


@pytest.mark.parametrize("B,Ci,T,Co,k,dil,act,res", CONV_CASES + [RAGGED])
def test_conv1d_bf16(lib, B, Ci, T, Co, k, dil, act, res):
    x, w, b = rnd((B, Ci, T), "cx"), rnd((Co, Ci, k), "cw", 1.0 / (Ci * k) ** 0.5), rnd((Co,), "cb")
    r = rnd((B, Co, T), "cr") if res else None
    pad = (k - 1) * dil // 2
    out = conv_bf16(lib, x, pack.pack_conv(w), b, B, Ci, T, Co, k, dil, pad, T, act=act, res=r)
    xin = F.leaky_relu(x.float(), 0.1) if act else x.float()
    ref = F.conv1d(r64(xin), r64(w), b.double(), dilation=dil, padding=pad)
    if res:
        ref = ref + r.double()
    assert rel_l2(out, ref) < TOL, describe("conv1d_bf16", out, ref)


@pytest.mark.parametrize("B,Ci,T,Co,k,u", [(2, 512, 24, 256, 16, 8), (1, 256, 33, 128, 15, 5), (1, 128, 20, 64, 11, 5),
                                          (2, 64, 50, 32, 4, 2), (1, 128, 19, 64, 8, 4)])
def test_conv_transpose1d_bf16(lib, B, Ci, T, Co, k, u):
    x, w, b = rnd((B, Ci, T), "tx"), rnd((Ci, Co, k), "tw", (u / (Ci * k)) ** 0.5), rnd((Co,), "tb")
    p = (k - u) // 2
    ref = F.conv_transpose1d(r64(F.leaky_relu(x.float(), 0.1)), r64(w), b.double(), stride=u, padding=p)
    T_out = ref.shape[-1]
    out = conv_bf16(lib, x, pack.pack_conv_transpose(w, u), b, B, Ci, T, Co, 0, 1, 0, T_out, tr=(u, p, k), act=1)
    assert rel_l2(out, ref) < TOL, describe("conv_transpose1d_bf16", out, ref)


def test_conv1d_bf16_groupnorm_swish(lib):
    """B = 1, Ci = 128, T = 37, Co = 64, k = 3: GroupNorm affine + swish fused into the staging.  The kernel's expf is not torch's: an
    activation that sits within a few fp32 ulps of a bf16 rounding boundary may round to the other side, a 2^-8 step that is no error of
    the convolution.  So the check has two halves.  (1) The kernel's own rounded activations are read back through an identity 1-tap
    convolution (one exact product per output, sums of zeros: exact) and each must be the bf16 rounding of a value within 8 fp32 ulps of the
    CPU's fp32 activation.  (2) The 3-tap convolution must sit within 2e-6 of the float64 convolution of THOSE activations."""
    B, Ci, T, Co, k, groups = 1, 128, 37, 64, 3, 32
    x, w, b = rnd((B, Ci, T), "gx").float(), rnd((Co, Ci, k), "gw", 1.0 / (Ci * k) ** 0.5), rnd((Co,), "gb")
    gamma, beta = (1.0 + 0.1 * rnd((Ci,), "gg")).float(), (0.1 * rnd((Ci,), "gbt")).float()
    xg = x.view(B, groups, -1)
    mean, rstd = xg.mean(-1).contiguous(), (xg.var(-1, unbiased=False) + 1e-6).rsqrt().contiguous()
    gn = (mean, rstd, gamma, beta, groups)
    eye = torch.eye(Ci).view(Ci, Ci, 1)
    got_act = conv_bf16(lib, x, pack.pack_conv(eye), None, B, Ci, T, Ci, 1, 1, 0, T, act=L.ACT_GN_SWISH, gn=gn).cpu()
    cpg = Ci // groups
    rs = rstd.repeat_interleave(cpg, 1) * gamma[None]
    sh = beta[None] - mean.repeat_interleave(cpg, 1) * rs
    t = (x.double() * rs.double()[..., None] + sh.double()[..., None]).float()       # the fused multiply-add, rounded once
    act = t / (1.0 + torch.exp(-t))
    slack = 8 * 2.0 ** -24 * act.abs()
    lo, hi = bf16_round(torch.minimum(act - slack, act + slack)), bf16_round(torch.maximum(act - slack, act + slack))
    assert bool(((got_act >= lo) & (got_act <= hi)).all()), describe("rounded activations", got_act, bf16_round(act))
    print(f"groupnorm + swish: {int((got_act != bf16_round(act)).sum())} of {act.numel()} activations round to the other side of a boundary")
    out = conv_bf16(lib, x, pack.pack_conv(w), b, B, Ci, T, Co, k, 1, 1, T, act=L.ACT_GN_SWISH, gn=gn)
    ref = F.conv1d(got_act.double(), r64(w), b.double(), padding=1)
    print(f"groupnorm + swish: rel_l2 {rel_l2(out, ref):.3e}")
    assert rel_l2(out, ref) < TOL, describe("conv1d_bf16 gn+swish", out, ref)


def test_conv1d_bf16_upsampled_input(lib):
    B, Ci, T, Co, k = 2, 96, 75, 96, 3
    x, w, b = rnd((B, Ci, T), "ux"), rnd((Co, Ci, k), "uw", 1.0 / (Ci * k) ** 0.5), rnd((Co,), "ub")
    out = conv_bf16(lib, x, pack.pack_conv(w), b, B, Ci, T, Co, k, 1, 1, 2 * T, upsample2=1)
    ref = F.conv1d(r64(x).repeat_interleave(2, dim=2), r64(w), b.double(), padding=1)
    assert rel_l2(out, ref) < TOL, describe("conv1d_bf16 upsample2", out, ref)


def test_conv1d_bf16_strided_pair_is_the_encoder_downsample(lib):
    """Downsample1D: pad right by one, k = 3, stride 2, as two polyphase launches (taps 0 and 2 over the even samples, tap 1 over the odd
    ones accumulated into the first result with beta = 1)"""
    B, C, T = 2, 96, 150
    x, w, b = rnd((B, C, T), "sx"), rnd((C, C, 3), "sw", 1.0 / (C * 3) ** 0.5), rnd((C,), "sb")
    out = conv_bf16(lib, x, pack.pack_conv(w[:, :, 0::2].contiguous()), b, B, C, T, C, 2, 1, 0, T // 2, in_stride=2, in_phase=0)
    out = conv_bf16(lib, x, pack.pack_conv(w[:, :, 1:2].contiguous()), None, B, C, T, C, 1, 1, 0, T // 2, in_stride=2, in_phase=1, beta=1.0, out=out)
    ref = F.conv1d(F.pad(r64(x), (0, 1)), r64(w), b.double(), stride=2)
    assert out.shape == ref.shape
    assert rel_l2(out, ref) < TOL, describe("conv1d_bf16 stride-2 pair", out, ref)


def test_conv1d_bf16_is_deterministic_on_a_ragged_shape(lib):
    B, Ci, T, Co, k, dil, _, _ = RAGGED
    x, w, b, r = rnd((B, Ci, T), "cx"), rnd((Co, Ci, k), "cw", 1.0 / (Ci * k) ** 0.5), rnd((Co,), "cb"), rnd((B, Co, T), "cr")
    outs = [conv_bf16(lib, x, pack.pack_conv(w), b, B, Ci, T, Co, k, dil, (k - 1) * dil // 2, T, act=1, res=r) for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- the fused pair
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 5), (7, 3), (11, 5)])
@pytest.mark.parametrize("T", [1000, 100])
@pytest.mark.parametrize("C", [32, 64])
def test_respair_bf16(lib, C, T, k, dil):
    """against the float64 restatement of the pair at (b) x 4, (b) = fp32- against float64-accumulated restatement of these very inputs;
    and against two vb_conv1d_bf16 launches within the same bound"""
    B, slope, alpha, beta = 2, 0.1, 1.0 / 3, 0.75
    x, old = rnd((B, C, T), "px").float(), rnd((B, C, T), "po").float()
    w1, w2 = rnd((C, C, k), "pw1", 1.0 / (C * k) ** 0.5).float(), rnd((C, C, k), "pw2", 1.0 / (C * k) ** 0.5).float()
    b1, b2 = rnd((C,), "pb1").float(), rnd((C,), "pb2").float()
    ref = pair_restatement(x, w1, b1, w2, b2, k, dil, slope, alpha, beta, old, torch.float64)
    b_num = rel_l2(pair_restatement(x, w1, b1, w2, b2, k, dil, slope, alpha, beta, old, torch.float32), ref)
    p1, _ = pack.pack_conv_bf16(pack.pack_conv(w1))
    p2, _ = pack.pack_conv_bf16(pack.pack_conv(w2))
    out = dev(old.clone())
    L.check(lib.vb_respair_bf16(L.ptr(dev(x)), L.ptr(dev(p1)), L.ptr(dev(b1)), L.ptr(dev(p2)), L.ptr(dev(b2)), B, C, T, k, dil, slope, alpha, beta,
                                L.ptr(out), L.stream_ptr()), "respair_bf16")
    sync()
    mid = conv_bf16(lib, x, pack.pack_conv(w1), b1, B, C, T, C, k, dil, (k - 1) * dil // 2, T, act=1, slope=slope)
    mid = torch.where(mid > 0, mid, mid * slope)
    two = conv_bf16(lib, mid.cpu(), pack.pack_conv(w2), b2, B, C, T, C, k, 1, (k - 1) // 2, T, res=x, alpha=alpha, beta=beta,
                    out=dev(old.clone()))
    e_ref, e_two = rel_l2(out, ref), rel_l2(out, two)
    print(f"respair_bf16 C={C} T={T} k={k} dil={dil}: (b) = {b_num:.3e}, pair vs restatement {e_ref:.3e}, pair vs two launches {e_two:.3e}")
    assert torch.isfinite(out).all()
    # (b) of ONE pair is a small-sample count: a handful of intermediates (none at T = 100 for most cases) cross a bf16 rounding boundary
    # between the fp32- and the float64-accumulated sums, each worth 2^-8 of itself.  The kernel's own handful is another draw of the same
    # count, so 4 x (b) is met with little room in places (C = 64, T = 1000, k = 7: 8.9e-6 against 9.0e-6) and would move with any change of
    # either side's summation order.  The bound is the issue's; what does not move is the second assertion.
    assert e_ref < 4 * b_num, describe("respair_bf16 vs restatement", out, ref)
    assert e_two < 4 * b_num, describe("respair_bf16 vs two conv1d_bf16 launches", out, two)
    # same chunk -> tap -> k-step order, same rounding point, same output arithmetic: not merely within the bound but the same bits
    assert torch.equal(out, two), describe("respair_bf16 vs two conv1d_bf16 launches, bit for bit", out, two)


@pytest.mark.parametrize("C,T,k,dil", [(32, 203, 7, 3), (64, 121, 3, 1), (64, 1001, 11, 5)])
def test_respair_bf16_direct_epilogue(lib, C, T, k, dil):
    """T % 4 != 0: rows are not 16-byte aligned and the pair (like the conv kernel) takes its direct 4-byte epilogue; one workgroup with a
    ragged tail / several.  Bit for bit the two launches, which test_conv1d_bf16 holds to the definition."""
    B, slope, alpha, beta = 2, 0.1, 0.5, 1.0
    x, old = rnd((B, C, T), "dx").float(), rnd((B, C, T), "do").float()
    w1, w2 = rnd((C, C, k), "dw1", 1.0 / (C * k) ** 0.5).float(), rnd((C, C, k), "dw2", 1.0 / (C * k) ** 0.5).float()
    b1, b2 = rnd((C,), "db1").float(), rnd((C,), "db2").float()
    p1, _ = pack.pack_conv_bf16(pack.pack_conv(w1))
    p2, _ = pack.pack_conv_bf16(pack.pack_conv(w2))
    out = dev(old.clone())
    L.check(lib.vb_respair_bf16(L.ptr(dev(x)), L.ptr(dev(p1)), L.ptr(dev(b1)), L.ptr(dev(p2)), L.ptr(dev(b2)), B, C, T, k, dil, slope, alpha, beta,
                                L.ptr(out), L.stream_ptr()), "respair_bf16")
    sync()
    mid = conv_bf16(lib, x, pack.pack_conv(w1), b1, B, C, T, C, k, dil, (k - 1) * dil // 2, T, act=1, slope=slope)
    mid = torch.where(mid > 0, mid, mid * slope)
    two = conv_bf16(lib, mid.cpu(), pack.pack_conv(w2), b2, B, C, T, C, k, 1, (k - 1) // 2, T, res=x, alpha=alpha, beta=beta, out=dev(old.clone()))
    ref = pair_restatement(x, w1, b1, w2, b2, k, dil, slope, alpha, beta, old, torch.float64)
    print(f"respair_bf16 direct epilogue C={C} T={T}: vs float64 restatement {rel_l2(out, ref):.3e}")
    assert torch.isfinite(out).all() and torch.equal(out, two), describe("respair_bf16 (direct epilogue) vs two launches", out, two)


# ---------------------------------------------------------------- nets
def _build_net(ctx, name, precision="bf16"):
    from versband_amd import engine
    sd, cfg, x, gold, _ = fixture_case(name)
    if name.startswith("hifigan_"):
        return engine.build_hifigan(ctx, sd, cfg.as_hparams(), precision=precision), x, gold
    if name.startswith("bigvgan_"):
        return engine.build_bigvgan(ctx, sd, cfg.as_hparams(), precision=precision), x, gold
    if name == "vae_decode":
        return engine.build_vae_decoder(ctx, sd, precision=precision), x, gold
    return engine.build_vae_encoder(ctx, sd, precision=precision), x, gold


@pytest.mark.parametrize("name", FIXTURES)
def test_nets_in_bf16_mode(ctx, name):
    net, x, gold = _build_net(ctx, name)
    out = net.run(x)
    sync()
    ref, a, b = restatement(name)
    e_ref, e_gold = rel_l2(out, ref), rel_l2(out, gold)
    print(f"{name} bf16: vs restatement {e_ref:.3e} (bound 4 x {b:.3e}), vs reference golden {e_gold:.3e} (bound 1.25 x {a:.3e})")
    assert out.shape == gold.shape and torch.isfinite(out).all()
    assert e_ref < 4 * b, describe(f"{name} bf16 vs restatement", out, ref)
    # Tightened from 2 x (a): one layer in another format is NOT separated by a factor of two - by no factor, see
    # test_bf16_mode.py::test_one_layer_in_another_format_is_not_separable_end_to_end.  The kernel's distance from the golden and (a) are
    # two draws of the same rounding noise over 10^4-10^6 output elements: equal norms up to a sampling fluctuation of a few per cent
    # (0.96-1.03 x (a) measured).  1.25 leaves that room and no more; a layer that is wrong, not merely rounded elsewhere, moves the
    # result by its own size.
    assert e_gold < 1.25 * a, describe(f"{name} bf16 vs reference", out, gold)


def test_hifigan_bf16_is_deterministic_and_not_the_split_mode(ctx):
    net, x, _ = _build_net(ctx, "hifigan_v1")
    o1 = net.run(x).clone()
    o2 = net.run(x).clone()
    sync()
    assert torch.equal(o1, o2)
    split, _, _ = _build_net(ctx, "hifigan_v1", "split")
    o3 = split.run(x)
    sync()
    assert not torch.equal(o1, o3)                 # (the mode really took its own kernels)


# ---------------------------------------------------------------- load-time refusals
def test_net_load_refuses_malformed_bf16_ops(ctx):
    lib = ctx.lib
    w = torch.zeros(65536, device=ctx.device)
    p = w.data_ptr()
    bufs = (L.BufDesc * 2)(L.BufDesc(32, 1, 0), L.BufDesc(128, 1, 0))

    def conv(**kw):
        f = dict(kind=L.OP_CONV, x=L.BUF_INPUT, out=0, res=-1, stats=-1, w_buf=-1, Ci=32, Co=32, ksize=3, dil=1, pad=1, alpha=1.0,
                 acc_scale=1.0, wfmt=L.WFMT_BF16, w_x3=p, ci_pad=32)
        f.update(kw)
        return L.NetOp(**f)

    def pair(**kw):
        f = dict(kind=L.OP_RESPAIR, x=0, out=L.BUF_OUTPUT, res=-1, stats=-1, w_buf=-1, Ci=32, Co=32, ksize=3, dil=1, alpha=1.0,
                 in_slope=0.1, wfmt=L.WFMT_BF16, w_x3=p, ci_pad=32, w2=p, bias=p, bias2=p)
        f.update(kw)
        return L.NetOp(**f)

    def load(op):
        ops = (L.NetOp * 2)(conv(), op)
        return lib.vb_net_load(ctx.handle, L.NET_VOCODER, ops, 2, bufs, 2, 32, 32, 1, 1)

    assert load(pair()) == 0
    assert load(conv(Ci=48, ci_pad=64)) == 0
    assert load(conv(x=0, out=L.BUF_OUTPUT, Co=1, w=p)) == 0            # one output channel: w is read
    cases = {
        "bad ci_pad": conv(Ci=48, ci_pad=48),
        "missing w_x3": conv(w_x3=None),
        "stray w_mf": conv(w_mf=p),
        "stray w on more than one output channel": conv(w=p),
        "pair with a bad ci_pad": pair(ci_pad=64),
        "pair without its second plane": pair(w2=None),
        "pair at C = 128": pair(x=1, out=1, Ci=128, Co=128, ci_pad=128),
    }
    for what, op in cases.items():
        assert load(op) == VB_E_INVALID, what
        msg = lib.vb_last_error().decode()
        assert "op 1" in msg, (what, msg)
