"""The conv nets' "bf16xt" precision on the GPU: the one-plane planes pre-pass, vb_conv1d_bf16_xt on both of its routes (the one-pass
conv-as-GEMM on the DMA-fed GEMM kernels, conv1d_bf16_kernel's DMA-fed input mode under VB_CONV_GEMM_OFF=1) against the float64 restatement
of one convolution with bf16-rounded operands, the net fixtures in bf16xt mode against the bounds of tests/test_bf16_mode.py ((b) x 4 and
(a) x 1.25, unchanged: they hold for any kernel that obeys the mode's definition), determinism, and vb_net_load's refusals of planes
buffers that do not match their reader."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import describe, rel_l2
from tests.test_bf16_mode import bf16_round, fixture_case, restatement
from tests.test_gpu_kernels import dev, rnd, sync
from versband_amd import _lib as L
from versband_amd import pack

pytestmark = pytest.mark.gpu
VB_E_INVALID = -1
TOL = 2e-6          # the project's bound for fp32-accumulating kernels (tests/test_gpu_kernels.py): only the accumulation order differs
HEAD, TAIL = 64, 384        # zero rows in front of / behind every clip of a planes buffer (include/versband_hip.h)
# the routes of a planes convolution: as launch_conv1d routes it (GEMM-eligible layers: the 64 x 64 DMA-fed tiles at these sizes), the same
# with the 128 x 128 DMA-fed kernel every batch of 8 clips runs (VB_GEMM_SMALL=0), and conv1d_bf16_kernel's DMA-fed input mode
ROUTES = {"routed": {}, "gemm128": {"VB_GEMM_SMALL": "0"}, "conv": {"VB_CONV_GEMM_OFF": "1"}}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    return Context("cuda:0")


@contextlib.contextmanager
def tuned(knobs):
    try:
        L.set_tuning(**knobs)
        yield
    finally:
        L.set_tuning(**{k: None for k in knobs})


def r64(t):
    return bf16_round(t.float()).double()


def gn_of(x, groups, tag):
    """GroupNorm statistics and affine of x [B][C][T] as the kernels take them"""
    B, C, _ = x.shape
    gamma, beta = (1.0 + 0.1 * rnd((C,), tag + "g")).float(), (0.1 * rnd((C,), tag + "b")).float()
    xg = x.view(B, groups, -1)
    return xg.mean(-1).contiguous(), (xg.var(-1, unbiased=False) + 1e-6).rsqrt().contiguous(), gamma, beta, groups


def conv_xt(lib, x, w, bias, k, dil, upsample2=0, act=0, slope=0.1, gn=None, res=None):
    """vb_conv1d_bf16_xt on x [B][Ci][T] with w [Co][Ci][k], 'same' padding -> (out [B][Co][T_eff], the plane scratch [B][T_eff + 448][Ci])"""
    B, Ci, T_in = x.shape
    Co, T_out, pad = w.shape[0], (2 * T_in if upsample2 else T_in), (k - 1) * dil // 2
    plane, cip = pack.pack_conv_bf16(pack.pack_conv(w))
    n = lib.vb_conv1d_bf16_xt_scratch_bytes(B, Ci, T_in, upsample2)
    assert n == B * (T_out + HEAD + TAIL) * Ci * 2
    scratch = torch.full((n // 2,), float("nan"), dtype=torch.bfloat16, device="cuda")
    out = torch.full((B, Co, T_out), float("nan"), device="cuda")
    gm, gr, gg, gb, groups = gn if gn is not None else (None, None, None, None, 0)
    L.check(lib.vb_conv1d_bf16_xt(L.ptr(dev(x)), L.ptr(dev(plane)), cip, L.ptr(dev(bias)) if bias is not None else None, B, Ci, T_in, Co, k, dil,
                                  pad, 1, 0, 0, T_out, upsample2, 1, 0, act, slope,
                                  L.ptr(dev(gm)) if gn else None, L.ptr(dev(gr)) if gn else None, L.ptr(dev(gg)) if gn else None,
                                  L.ptr(dev(gb)) if gn else None, groups, L.ptr(dev(res)) if res is not None else None, 1.0, 0.0, L.ptr(out),
                                  L.ptr(scratch), L.stream_ptr()), "conv1d_bf16_xt")
    sync()
    return out, scratch.view(B, T_out + HEAD + TAIL, Ci)


def planes(lib, x, nplanes, upsample2=0, act=0, slope=0.1, gn=None):
    """vb_xt_planes -> [nplanes][B][T_eff + 448][C] bf16"""
    B, C, T_in = x.shape
    n = lib.vb_xt_planes_bytes(B, C, T_in, upsample2, nplanes)
    buf = torch.full((n // 2,), float("nan"), dtype=torch.bfloat16, device="cuda")
    gm, gr, gg, gb, groups = gn if gn is not None else (None, None, None, None, 0)
    L.check(lib.vb_xt_planes(L.ptr(dev(x)), B, C, T_in, upsample2, act, slope, L.ptr(dev(gm)) if gn else None, L.ptr(dev(gr)) if gn else None,
                             L.ptr(dev(gg)) if gn else None, L.ptr(dev(gb)) if gn else None, groups, nplanes, L.ptr(buf), L.stream_ptr()), "xt_planes")
    sync()
    return buf.view(nplanes, B, -1, C).cpu()


def interior(plane_btc):
    """the clip rows of a plane [B][T_eff + 448][C] as [B][C][T_eff] float"""
    return plane_btc[:, HEAD:plane_btc.shape[1] - TAIL].float().transpose(1, 2).contiguous()


# B, Ci, T, Co, k, dil, what else
SHAPES = {
    "gemm_bias_res": (2, 64, 100, 384, 3, 1, "res"),          # GEMM route; tiles ragged against the per-clip row groups; halo rows at both clip ends
    "ragged_n_gn_swish": (1, 128, 37, 388, 1, 1, "gn"),       # Co % 4 == 0 but no tile multiple; T below one tile; GroupNorm + swish in the pre-pass
    "upsampled": (2, 64, 24, 384, 3, 1, "up"),
    "dilated_3_chunks": (1, 192, 200, 384, 3, 2, ""),          # dilation; three 64-channel K chunks per tap
    "ci_96": (2, 96, 100, 384, 3, 1, ""),                      # Ci % 64 != 0: not GEMM-eligible, a 32-channel last chunk in the conv kernel
}


def _case(name):
    B, Ci, T, Co, k, dil, extra = SHAPES[name]
    x, w, b = rnd((B, Ci, T), name + "x").float(), rnd((Co, Ci, k), name + "w", 1.0 / (Ci * k) ** 0.5).float(), rnd((Co,), name + "b").float()
    up = 1 if extra == "up" else 0
    kw = dict(upsample2=up)
    if extra == "res":
        kw["res"] = rnd((B, Co, T), name + "r").float()
    if extra == "gn":
        kw.update(act=L.ACT_GN_SWISH, gn=gn_of(x, 32, name))
    return x, w, b, k, dil, kw


@pytest.mark.parametrize("name", list(SHAPES))
def test_conv1d_bf16_xt_on_every_route(lib, name):
    """each route within 2e-6 of the float64 convolution of the bf16-rounded operands.  GroupNorm + swish: the kernel's expf is not torch's,
    so (as test_conv1d_bf16_groupnorm_swish does) the pre-pass's own rounded activations - here simply read back from the plane - must each be
    the bf16 rounding of a value within 8 fp32 ulps of the CPU's activation, and the convolution is held to 2e-6 of the float64 convolution
    of THOSE activations."""
    x, w, b, k, dil, kw = _case(name)
    pad = (k - 1) * dil // 2
    for route, knobs in ROUTES.items():
        with tuned(knobs):
            out, plane = conv_xt(lib, x, w, b, k, dil, **kw)
        got_act = interior(plane.cpu())
        if kw.get("gn"):
            mean, rstd, gamma, beta, groups = kw["gn"]
            cpg = x.shape[1] // groups
            rs = rstd.repeat_interleave(cpg, 1) * gamma[None]
            sh = beta[None] - mean.repeat_interleave(cpg, 1) * rs
            t = (x.double() * rs.double()[..., None] + sh.double()[..., None]).float()
            act = t / (1.0 + torch.exp(-t))
            slack = 8 * 2.0 ** -24 * act.abs()
            lo, hi = bf16_round(torch.minimum(act - slack, act + slack)), bf16_round(torch.maximum(act - slack, act + slack))
            assert bool(((got_act >= lo) & (got_act <= hi)).all()), describe("rounded activations", got_act, bf16_round(act))
            xin = got_act.double()
        else:
            xin = r64(x.repeat_interleave(2, dim=2) if kw.get("upsample2") else x)
            assert torch.equal(got_act.double(), xin), "the plane is not the bf16 rounding of the (upsampled) input"
        ref = F.conv1d(xin, r64(w), b.double(), dilation=dil, padding=pad)
        if kw.get("res") is not None:
            ref = ref + kw["res"].double()
        err = rel_l2(out, ref)
        print(f"conv1d_bf16_xt {name} [{route}]: rel_l2 {err:.3e}")
        assert torch.isfinite(out).all() and err < TOL, describe(f"conv1d_bf16_xt {name} [{route}]", out, ref)


@pytest.mark.parametrize("name", ["gemm_bias_res", "upsampled"])
def test_one_plane_is_plane_0_of_the_split_planes(lib, name):
    x, _, _, _, _, kw = _case(name)
    up = kw["upsample2"]
    one, two = planes(lib, x, 1, upsample2=up), planes(lib, x, 2, upsample2=up)
    assert one.shape[0] == 1 and two.shape[0] == 2 and one.shape[1:] == two.shape[1:]
    assert one.shape[2] == (2 if up else 1) * x.shape[2] + HEAD + TAIL
    assert torch.equal(one[0].view(torch.int16), two[0].view(torch.int16))          # bit for bit, halo rows included
    assert bool((one[0][:, :HEAD] == 0).all()) and bool((one[0][:, -TAIL:] == 0).all())
    xin = x.repeat_interleave(2, dim=2) if up else x
    assert torch.equal(interior(one[0]), bf16_round(xin))
    assert torch.equal(interior(two[1]), bf16_round(xin - bf16_round(xin)))         # (the split form still writes its residual plane)


def test_conv1d_bf16_xt_is_deterministic_on_each_route(lib):
    x, w, b, k, dil, kw = _case("gemm_bias_res")
    for route, knobs in ROUTES.items():
        with tuned(knobs):
            o1, _ = conv_xt(lib, x, w, b, k, dil, **kw)
            o2, _ = conv_xt(lib, x, w, b, k, dil, **kw)
        assert torch.isfinite(o1).all() and torch.equal(o1, o2), route


# ---------------------------------------------------------------- nets
def _build_net(ctx, name, precision="bf16xt"):
    from versband_amd import engine
    sd, cfg, x, gold, _ = fixture_case(name)
    if name.startswith("hifigan_"):
        return engine.build_hifigan(ctx, sd, cfg.as_hparams(), precision=precision), x, gold
    if name.startswith("bigvgan_"):
        return engine.build_bigvgan(ctx, sd, cfg.as_hparams(), precision=precision), x, gold
    if name == "vae_decode":
        return engine.build_vae_decoder(ctx, sd, precision=precision), x, gold
    return engine.build_vae_encoder(ctx, sd, precision=precision), x, gold


def _check_net(name, out, gold, what):
    ref, a, b = restatement(name)
    e_ref, e_gold = rel_l2(out, ref), rel_l2(out, gold)
    print(f"{name} {what}: vs restatement {e_ref:.3e} (bound 4 x {b:.3e}), vs reference golden {e_gold:.3e} (bound 1.25 x {a:.3e})")
    assert out.shape == gold.shape and torch.isfinite(out).all()
    assert e_ref < 4 * b, describe(f"{name} {what} vs restatement", out, ref)
    assert e_gold < 1.25 * a, describe(f"{name} {what} vs reference", out, gold)


@pytest.mark.parametrize("name", ["vae_decode", "vae_encode", "hifigan_v1", "bigvgan_amp1"])
def test_nets_in_bf16xt_mode(ctx, name):
    net, x, gold = _build_net(ctx, name)
    out = net.run(x)
    sync()
    _check_net(name, out, gold, "bf16xt")


def test_vae_decode_bf16xt_gemm_route_on_and_off(ctx):
    """both routes of the planes layers inside the bounds, each deterministic; the two are different accumulation orders and need not be equal"""
    net, x, gold = _build_net(ctx, "vae_decode")
    assert any(o.kind == L.OP_XT_PLANES and o.wfmt == L.WFMT_BF16 for o in net.nb.ops)
    outs = {}
    for route in ("routed", "conv"):
        with tuned(ROUTES[route]):
            o1 = net.run(x).clone()
            o2 = net.run(x).clone()
            sync()
        assert torch.equal(o1, o2), route
        _check_net("vae_decode", o1, gold, f"bf16xt [{route}]")
        outs[route] = o1
    print(f"vae_decode bf16xt, GEMM route vs conv kernel: rel_l2 {rel_l2(outs['routed'], outs['conv']):.3e}")


# ---------------------------------------------------------------- load-time refusals
def test_net_load_refuses_planes_that_do_not_match_their_reader(ctx):
    lib = ctx.lib
    w = torch.zeros(1 << 20, device=ctx.device)
    p = w.data_ptr()
    C = 384
    bufs = (L.BufDesc * 3)(L.BufDesc(C, 1, 3), L.BufDesc(C, 1, 4), L.BufDesc(C, 1, 0))       # split planes, one plane, a plain buffer

    def planes_op(out, wfmt):
        return L.NetOp(kind=L.OP_XT_PLANES, wfmt=wfmt, x=L.BUF_INPUT, out=out, res=-1, stats=-1, w_buf=-1, Ci=C, gn_groups=32)

    def conv(x, wfmt, **kw):
        f = dict(kind=L.OP_CONV, x=x, out=L.BUF_OUTPUT, res=-1, stats=-1, w_buf=-1, Ci=C, Co=C, ksize=3, dil=1, pad=1, alpha=1.0, acc_scale=1.0,
                 wfmt=wfmt, w_x3=p, ci_pad=C, x_planes=1)
        if wfmt == L.WFMT_X3:
            f["w"] = p
        f.update(kw)
        return L.NetOp(**f)

    def load(first, second, out_ch=C):
        ops = (L.NetOp * 2)(first, second)
        return lib.vb_net_load(ctx.handle, L.NET_VAE, ops, 2, bufs, 3, C, out_ch, 1, 1)

    assert load(planes_op(0, L.WFMT_NONE), conv(0, L.WFMT_X3)) == 0
    assert load(planes_op(1, L.WFMT_BF16), conv(1, L.WFMT_BF16)) == 0
    cases = {
        "split planes into a BF16 conv": (planes_op(0, L.WFMT_NONE), conv(0, L.WFMT_BF16), C),
        "one plane into an X3 conv": (planes_op(1, L.WFMT_BF16), conv(1, L.WFMT_X3), C),
        "one plane into a BF16 conv of one output channel": (planes_op(1, L.WFMT_BF16), conv(1, L.WFMT_BF16, Co=1, w=p), 1),
        "a plain buffer read as planes": (planes_op(1, L.WFMT_BF16), conv(2, L.WFMT_BF16), C),
    }
    for what, (first, second, out_ch) in cases.items():
        assert load(first, second, out_ch) == VB_E_INVALID, what
        msg = lib.vb_last_error().decode()
        assert "op 1" in msg, (what, msg)
    # the pre-pass itself: the one-plane form writes a one-plane buffer, the split form a two-plane one
    for first in (planes_op(0, L.WFMT_BF16), planes_op(1, L.WFMT_NONE)):
        assert load(first, conv(1, L.WFMT_BF16)) == VB_E_INVALID
        assert "op 0" in lib.vb_last_error().decode()
