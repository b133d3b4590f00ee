"""Float64 oracles of the convolution and ResBlock-pair kernels, one launch at a time, each with a derived per-element error bound
(plain torch, CPU).  Constants and acc(K) as in tests/moe_oracles.py (U32 = 2^-24, UB = 2^-8, acc(K) = 2 K U32: fp32 accumulation of K
products in any order, relative to sum |x_k| |w_k|).

Every oracle is evaluated on the operand values the kernel multiplies.  The input transform the unit ABI reaches without device
statistics is LeakyReLU, one fp32 multiplication `x * slope`: the oracle does that one multiplication in float32 too, so the activated
operand is the kernel's, bit for bit, and the bf16 roundings behind it round the same value (no neighbouring-bf16 term is needed).
GroupNorm (+ swish) inputs (one-plane kernels and the planes pre-pass): the device forms t = x rs + sh in fp32 and swish with a fast
exponential, so its value may land on the neighbouring bf16 of the float64 one.  Of the two ways the bound may cover that, the UB S way is
used (as band_ffn in moe_oracles.py): E gains UB S - every activation of the window off by half the largest bf16 spacing at once - and
4.4 U32 conv(|x rs| + |sh|, |w|) for the fp32 evaluation of t where x rs and sh cancel (swish has slope <= 1.1).
With xa the activated input after nearest-x2 upsampling / strided reading, zero outside the clip, and S = conv(|xa|, |w|) over the taps
that exist for the output (a transposed convolution's phase has ceil(k / u) of them at most), all bounds are first order and relative
to S, not to the result, so cancellation is covered:

  exact fp32 (CONV_F32, CONV_F32G, CONV_CO1)      E = acc(Ci taps) S                 operands xa, w
  split bf16 (CONV_X3)                            E = (acc(3 Ci_pad taps) + UB^2) S   operands hi + lo of xa and of w: three of the four
                                                                                      plane products are summed, lo x lo (<= UB^2 |x| |w|) is not
  one plane bf16 (CONV_BF16, CONV_BF16_XT, GEMM)  E = acc(Ci_pad taps) S              operands bf16(xa), bf16(w): products exact in fp32
  minimal filtering (CONV_F32W)                   E = (acc(Ci P) + 3 U32) S_mf        see below

The epilogue actually executed (conv1d_dev.h: conv_out_value; acc_scale is 1 and there is no output activation behind the unit ABI)
is v = (a + bias) + res, out = fma(v, alpha, beta * old): two additions, the product beta * old and the fused multiply-add round once each,
    bound = |alpha| (E + U32 (|a + bias| + |a + bias + res|)) + U32 |beta old| + U32 |out|.

Minimal filtering.  F(2,3) forms two outputs dil apart from four accumulators (mf_taps.h): pseudo-tap j multiplies a difference / sum /
copy of two window values (one rounding, U32 |operand|) with a pre-combined weight (pack.pack_conv_mf) into accumulator acc(j), and
    y_even = A0 + A1 + A2,    y_odd = A1 - A2 - A3          (two roundings, <= 2 U32 (|A0| + |A1| + |A2|) <= 2 U32 S_mf)
with S_mf = sum over the member's three accumulators of |operand| |packed w|.  Which member an output position is depends on where the
kernel's tile starts, which the oracle does not model: it evaluates BOTH forms at every position in float64 on the packed weights, takes
the larger S_mf, and returns the plain convolution beside them - the test asserts that all three agree to 1e-12 S, which checks the
packing and the table.  That needs the packed combinations to be exact in fp32, so the weights of these cases lie on a 2^-16 grid
((w0 + w1 + w2) / 2 then has at most 19 significant bits).

Pairs (respair_dev.h): out = beta out_in + alpha (x + b2 + conv2_{k,1}(h)),  h = lrelu(b1 + conv1_{k,dil}(lrelu(x))), zero outside [0, T).
The first stage errs by e1 = E1 + U32 (|a1 + b1| + |h|) (bias addition, LeakyReLU, slope <= 1 so the error does not grow), which reaches the
output through conv(e1, |w2|); the second stage's own error is taken on S2 = conv(|h| + e1, |w2|).  bf16 pair: both sides round the
intermediate to bf16, values e1 apart land at most e1 + UB (2 |h| + e1) apart (moe_oracles.py); split pair: hi + lo represents the
intermediate to UB^2.

Inputs come from versband_amd.prng: weights scaled by 1 / sqrt(Ci k); every clip's first and last `halo` columns are 8 x the interior, so
a lost or doubled edge tap stands clear of the bound; the last clip of a batch is quiet (/ 64), where a leaked neighbour value weighs
like a real one."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.moe_oracles import U32, UB, acc, bf16r
from versband_amd import pack, prng

SLOPE = 0.1
# routes of vb_conv1d_plan (include/versband_hip.h: VB_ROUTE_*)
AS_GEMM, F32W, CO1, BF16_XT, BF16, X3_XT, X3, F32G, F32 = range(9)
W_F32, W_MF, W_X3, W_BF16 = 1, 2, 4, 8
X_4B, OUT_4B, RES_4B = 1, 2, 4
PAIR_F32, PAIR_MF, PAIR_X3, PAIR_BF16 = range(4)


def rnd(shape, name, scale=1.0) -> torch.Tensor:
    n = int(np.prod(shape))
    return (torch.from_numpy(prng.normal(prng.key_seed(13, name), n).reshape(shape)) * scale).float()


def worst(err, bound) -> float:
    return float((err / bound).max())


def case(fam, B, Ci, T, Co, k, dil, plan, pad=None, T_out=None, tr=None, ups=0, stride=1, phase=0, act=1, res=False, alpha=1.0, beta=0.0,
         mis=0, knobs=None, gn=None):
    """one convolution call.  fam: 'f32' | 'mf' | 'x3' | 'x3xt' | 'bf16' | 'bf16xt'; gn = (groups, swish): GroupNorm (+ swish) input transform; tr = (u, k_tr) for a transposed convolution (pad (k - u) / 2);
    plan = (route, tile_co, tile_t) the call must be planned as; mis = operands passed 4-byte aligned; knobs = VB_* switches of the case"""
    c = dict(fam=fam, B=B, Ci=Ci, T=T, Co=Co, k=k, dil=dil, tr=tr, ups=ups, stride=stride, phase=phase, act=act, res=res,
             alpha=float(np.float32(alpha)), beta=float(np.float32(beta)), mis=mis, plan=plan, knobs=knobs or {}, gn=gn)
    if gn:
        c["act"] = 2 if gn[1] else 4          # (ACT_GN_SWISH / ACT_GN of csrc/kernels.h)
    T_eff = 2 * T if ups else (T - phase + stride - 1) // stride
    if tr:
        u, kt = tr
        c.update(k=0, dil=1, pad=0, u=u, tr_k=kt, tr_pad=(kt - u) // 2, ntaps=(kt + u - 1) // u)
        c["T_out"] = T_out if T_out is not None else (T - 1) * u - 2 * c["tr_pad"] + kt
    else:
        c.update(u=1, tr_k=0, tr_pad=0, ntaps=k, pad=(k - 1) * dil // 2 if pad is None else pad)
        c["T_out"] = T_out if T_out is not None else T_eff + 2 * c["pad"] - (k - 1) * dil
    c["T_eff"] = T_eff
    c["halo"] = (c["ntaps"] - 1) * dil
    c["Ci_pad"] = (Ci + 31) // 32 * 32
    c["wforms"] = {"f32": W_F32, "mf": W_F32 | W_MF, "x3": W_F32 | W_X3, "bf16": W_BF16, "bf16xt": W_BF16, "x3xt": W_X3}[fam]
    c["xt"] = int(fam in ("bf16xt", "x3xt"))
    c["id"] = f"{fam}-B{B}-Ci{Ci}-T{T}-Co{Co}-k{tr[1] if tr else k}" + (f"u{tr[0]}" if tr else f"d{dil}p{c['pad']}") + \
        (f"-o{c['T_out']}" if T_out is not None else "") + ("-ups" if ups else "") + (f"-s{stride}.{phase}" if stride > 1 else "") + \
        ("" if act else "-noact") + (f"-gn{gn[0]}{'s' if gn[1] else ''}" if gn else "") + ("-res" if res else "") + (f"-ab{alpha:.2f}.{beta:g}" if (alpha, beta) != (1.0, 0.0) else "") + \
        (f"-mis{mis}" if mis else "") + "".join(f"-{a[3:]}" for a in c["knobs"])
    return c


def edged(x, halo):
    """every clip's first and last `halo` (>= 1) columns 8 x, the last clip of a batch of two or more quiet (/ 64)"""
    x = x.clone()
    h = max(1, min(halo, x.shape[-1]))
    x[..., :h] *= 8
    if x.shape[-1] > h:
        x[..., -h:] *= 8
    if x.shape[0] >= 2:
        x[-1] /= 64
    return x


def conv_inputs(c):
    """x [B][Ci][T], w (torch layout: [Co][Ci][k], transposed [Ci][Co][k]), b [Co], res / out_in [B][Co][T_out] (None where the call has none)"""
    kk = c["tr_k"] if c["tr"] else c["k"]
    sc = (c["u"] / (c["Ci"] * kk)) ** 0.5
    w = rnd((c["Ci"], c["Co"], kk) if c["tr"] else (c["Co"], c["Ci"], kk), "w" + c["id"], sc)
    if c["fam"] == "mf":
        w = torch.round(w * 65536) / 65536
    o = (c["B"], c["Co"], c["T_out"])
    gn = {}
    if c["gn"]:      # statistics of the clip as launch_gn_stats defines them (eps 1e-6), computed on the host in fp32
        x = edged(rnd((c["B"], c["Ci"], c["T"]), "x" + c["id"]), c["halo"])
        xg = x.view(c["B"], c["gn"][0], -1)
        gn = dict(mean=xg.mean(-1).contiguous(), rstd=(xg.var(-1, unbiased=False) + 1e-6).rsqrt().contiguous(),
                  gamma=(1.0 + 0.1 * rnd((c["Ci"],), "g" + c["id"])).float(), gbeta=(0.1 * rnd((c["Ci"],), "h" + c["id"])).float())
    return dict(gn, x=edged(rnd((c["B"], c["Ci"], c["T"]), "x" + c["id"]), c["halo"] * c["stride"] // (2 if c["ups"] else 1)), w=w,
                b=rnd((c["Co"],), "b" + c["id"], 0.5), res=edged(rnd(o, "r" + c["id"]), 1) if c["res"] else None,
                out_in=edged(rnd(o, "o" + c["id"]), 1) if c["beta"] != 0.0 else None)


def lrelu32(x):
    """the kernels' LeakyReLU: one fp32 multiplication"""
    x = x.float()
    return torch.where(x > 0, x, x * np.float32(SLOPE))


def gn_affine(c, inp):
    """(scale, shift) fp32 [B][Ci][1] of the folded GroupNorm affine, as the kernels form them: rs = rstd * gamma, sh = beta - mean * rs"""
    cpg = c["Ci"] // c["gn"][0]
    rs = inp["rstd"].repeat_interleave(cpg, 1) * inp["gamma"][None]
    sh = inp["gbeta"][None] - inp["mean"].repeat_interleave(cpg, 1) * rs
    return rs[..., None], sh[..., None]


def activated(c, x, inp=None, dtype=torch.float32):
    """xa [B][Ci][T_eff]: the convolution's input after the pointwise transform and the upsampled / strided reading (fp32: the kernels' own
    LeakyReLU; GroupNorm: x rs + sh (+ swish) evaluated in `dtype`)"""
    if c["gn"]:
        rs, sh = gn_affine(c, inp)
        t = x.to(dtype) * rs.to(dtype) + sh.to(dtype)
        xa = t / (1.0 + torch.exp(-t)) if c["gn"][1] else t
    else:
        xa = lrelu32(x) if c["act"] == 1 else x.float()
    if c["ups"]:
        xa = xa.repeat_interleave(2, dim=-1)
    if c["stride"] > 1:
        xa = xa[..., c["phase"]::c["stride"]]
    return xa.contiguous()


def split(v):
    """fp32 -> (hi, lo) bf16 planes as float64"""
    v = v.float()
    hi = v.bfloat16().float()
    return hi.double(), (v - hi).bfloat16().double()


def raw_conv(c, xa, w):
    """the convolution alone: xa [B][Ci][T_eff], w torch layout (any float dtype) -> [B][Co][T_out]"""
    if c["tr"]:
        nat = (xa.shape[-1] - 1) * c["u"] - 2 * c["tr_pad"] + c["tr_k"]
        y = F.conv_transpose1d(xa, w, stride=c["u"], padding=c["tr_pad"], output_padding=max(0, min(c["u"] - 1, c["T_out"] - nat)))
        return y[..., :c["T_out"]]
    padr = c["T_out"] - 1 - c["pad"] + (c["ntaps"] - 1) * c["dil"] - (xa.shape[-1] - 1)      # zero columns the last output reads behind the clip
    y = F.conv1d(F.pad(xa, (c["pad"], max(0, padr))), w, dilation=c["dil"])[..., :c["T_out"]]
    assert y.shape[-1] == c["T_out"], (y.shape, c["T_out"])
    return y


def operands(c, inp):
    """(xo, wo) float64: the values the family's kernel multiplies"""
    xa, w = activated(c, inp["x"], inp, torch.float64 if c["gn"] else torch.float32), inp["w"].float()
    if c["fam"] in ("f32", "mf"):
        return xa.double(), w.double()
    if c["fam"] in ("x3", "x3xt"):
        (xh, xl), (wh, wl) = split(xa), split(w)
        return xh + xl, wh + wl
    return bf16r(xa.double()), bf16r(w.double())


def acc_factor(c):
    """E / S of the family's accumulation (module docstring)"""
    if c["fam"] in ("x3", "x3xt"):
        return acc(3 * c["Ci_pad"] * c["ntaps"]) + UB * UB
    if c["fam"] in ("bf16", "bf16xt"):
        return acc(c["Ci_pad"] * c["ntaps"])
    return acc(c["Ci"] * c["ntaps"])


def epilogue(a, E, b, res, out_in, alpha, beta):
    """(ref, bound) of out = fma((a + b) + res, alpha, beta * old) around an accumulator a known to E"""
    v1 = a + b.double().view(1, -1, 1)
    v2 = v1 + (res.double() if res is not None else 0.0)
    old = beta * out_in.double() if out_in is not None else torch.zeros_like(a)
    ref = alpha * v2 + old
    return ref, abs(alpha) * (E + U32 * (v1.abs() + v2.abs())) + U32 * old.abs() + U32 * ref.abs()


# ---- minimal filtering ------------------------------------------------------------------------------------------------------------------
def mf_tap(K, j):
    """(acc, op, oa, ob) of pseudo-tap j: the table of csrc/mf_taps.h"""
    ng, o = K // 3, 3 * (j // 4)
    if j < 4 * ng:
        return [(0, 0, o, o + 2), (1, 1, o + 1, o + 2), (2, 0, o + 2, o + 1), (3, 0, o + 1, o + 3)][j & 3]
    r, ob = j - 4 * ng, 3 * ng
    if K % 3 == 1:
        return (0, 2, ob, ob) if r == 0 else (3, 2, ob + 1, ob + 1)
    return (0, 0, ob, ob + 1) if r == 0 else ((1, 2, ob + 1, ob + 1) if r == 1 else (3, 0, ob + 2, ob + 1))


def mf_accumulators(xa, wmf, k, dil, pad, T_out, dtype=torch.float64):
    """A [4][B][Co][T_out + dil] and the matching sums of |operand| |w|: entry m belongs to the pair whose even output is m - dil"""
    B, Ci, T = xa.shape
    n = T_out + dil
    xp = F.pad(xa.to(dtype), (pad + dil, n + (k + 1) * dil))
    A = torch.zeros(4, B, wmf.shape[2], n, dtype=dtype)
    S = torch.zeros_like(A)
    for j in range(wmf.shape[0]):
        a, op, oa, ob = mf_tap(k, j)
        xa_, xb_ = xp[..., oa * dil:oa * dil + n], xp[..., ob * dil:ob * dil + n]
        v = xa_ - xb_ if op == 0 else (xa_ + xb_ if op == 1 else xa_)
        wj = wmf[j].to(dtype)
        A[a] += torch.einsum("bct,co->bot", v, wj)
        S[a] += torch.einsum("bct,co->bot", v.abs(), wj.abs())
    return A, S


def mf_forms(A, S, dil):
    """-> (y as even member, y as odd member, S_mf as even, S_mf as odd) per output position"""
    ev, od = slice(dil, None), slice(0, A.shape[-1] - dil)
    return (A[0] + A[1] + A[2])[..., ev], (A[1] - A[2] - A[3])[..., od], (S[0] + S[1] + S[2])[..., ev], (S[1] + S[2] + S[3])[..., od]


def mf_stage(xo, w, k, dil, pad, T_out, Ci):
    """(a, E, plain, S, worst disagreement / S of the three float64 evaluations) of one minimal-filtering convolution"""
    wmf = pack.pack_conv_mf(w.float())
    A, Sm = mf_accumulators(xo, wmf, k, dil, pad, T_out)
    ye, yo, se, so = mf_forms(A, Sm, dil)
    plain = F.conv1d(xo, w.double(), dilation=dil, padding=pad)
    S = F.conv1d(xo.abs(), w.double().abs(), dilation=dil, padding=pad)
    dis = float((torch.maximum((ye - plain).abs(), (yo - plain).abs()) / S.clamp_min(1e-300)).max())
    E = (acc(Ci * wmf.shape[0]) + 3 * U32) * torch.maximum(se, so) + 0.5 * (ye - yo).abs()
    return 0.5 * (ye + yo), E, plain, S, dis


# ---- one convolution ----------------------------------------------------------------------------------------------------------------------
def conv_reference(c, inp):
    """-> (ref, bound) float64 [B][Co][T_out]; for the minimal-filtering family also c['mf_disagreement'] (module docstring)"""
    xo, wo = operands(c, inp)
    if c["fam"] == "mf":
        a, E, _, _, c["mf_disagreement"] = mf_stage(xo, inp["w"], c["k"], c["dil"], c["pad"], c["T_out"], c["Ci"])
    else:
        S = raw_conv(c, xo.abs(), wo.abs())
        a, E = raw_conv(c, xo, wo), acc_factor(c) * S
        if c["gn"]:      # the UB S way (module docstring), and the fp32 evaluation of x rs + sh where it cancels
            rs, sh = gn_affine(c, inp)
            mag = (inp["x"].double() * rs.double()).abs() + sh.double().abs()
            E = E + UB * S + 4.4 * U32 * raw_conv(c, mag.expand_as(xo), wo.abs())
    return epilogue(a, E, inp["b"], inp["res"], inp["out_in"], c["alpha"], c["beta"])


def conv_emulation(c, inp):
    """the kernel's arithmetic in float32 torch (another summation order, the same operand roundings and epilogue) -> fp32 [B][Co][T_out]"""
    xa, w = activated(c, inp["x"], inp), inp["w"].float()
    if c["fam"] == "mf":
        A, _ = mf_accumulators(xa, pack.pack_conv_mf(w), c["k"], c["dil"], c["pad"], c["T_out"], torch.float32)
        ye, yo, _, _ = mf_forms(A, torch.zeros_like(A), c["dil"])
        t = torch.arange(c["T_out"])
        a = torch.where((t // c["dil"]) % 2 == 0, ye, yo)
    elif c["fam"] in ("x3", "x3xt"):
        (xh, xl), (wh, wl) = split(xa), split(w)
        xh, xl, wh, wl = xh.float(), xl.float(), wh.float(), wl.float()
        a = raw_conv(c, xl, wh) + raw_conv(c, xh, wl) + raw_conv(c, xh, wh)
    elif c["fam"] == "f32":
        a = raw_conv(c, xa, w)
    else:
        a = raw_conv(c, xa.bfloat16().float(), w.bfloat16().float())
    v = a + inp["b"].view(1, -1, 1)
    if inp["res"] is not None:
        v = v + inp["res"]
    al, be = np.float32(c["alpha"]), np.float32(c["beta"])
    return v * al + (inp["out_in"] * be if inp["out_in"] is not None else 0.0)


# ---- pairs ---------------------------------------------------------------------------------------------------------------------------------
def pair_case(form, B, C, T, k, dil, alpha=1.0, beta=0.0, knobs=None):
    fam = {PAIR_F32: "f32", PAIR_MF: "mf", PAIR_X3: "x3", PAIR_BF16: "bf16"}[form]
    return dict(form=form, fam=fam, B=B, C=C, T=T, k=k, dil=dil, alpha=float(np.float32(alpha)), beta=float(np.float32(beta)),
                halo=(k - 1) * dil, knobs=knobs or {}, id=f"pair-{fam}-B{B}-C{C}-T{T}-k{k}d{dil}" +
                (f"-ab{alpha:.2f}.{beta:g}" if (alpha, beta) != (1.0, 0.0) else ""))


def pair_inputs(c):
    C, k = c["C"], c["k"]
    w1, w2 = rnd((C, C, k), "w1" + c["id"], (C * k) ** -0.5), rnd((C, C, k), "w2" + c["id"], (C * k) ** -0.5)
    if c["fam"] == "mf":
        w1, w2 = torch.round(w1 * 65536) / 65536, torch.round(w2 * 65536) / 65536
    o = (c["B"], C, c["T"])
    return dict(x=edged(rnd(o, "x" + c["id"]), c["halo"] // 2 + k // 2), w1=w1, w2=w2, b1=rnd((C,), "b1" + c["id"], 0.5), b2=rnd((C,), "b2" + c["id"], 0.5),
                out_in=edged(rnd(o, "o" + c["id"]), 1) if c["beta"] != 0.0 else None)


def _pair_stage(c, xin, w, dil):
    """(a, E, S) of one convolution of the pair on its fp32 input values (already activated)"""
    C, k, fam = c["C"], c["k"], c["fam"]
    pad = (k - 1) * dil // 2
    if fam == "mf":
        a, E, plain, S, dis = mf_stage(xin.double(), w, k, dil, pad, xin.shape[-1], C)
        c["mf_disagreement"] = max(c.get("mf_disagreement", 0.0), dis)
        return a, E, S
    if fam == "x3":
        (xh, xl), (wh, wl) = split(xin), split(w)
        xo, wo, f = xh + xl, wh + wl, acc(3 * C * k) + UB * UB
    elif fam == "bf16":
        xo, wo, f = bf16r(xin.double()), bf16r(w.double()), acc(C * k)
    else:
        xo, wo, f = xin.double(), w.double(), acc(C * k)
    S = F.conv1d(xo.abs(), wo.abs(), dilation=dil, padding=pad)
    return F.conv1d(xo, wo, dilation=dil, padding=pad), f * S, S


def pair_reference(c, inp):
    """-> (ref, bound) float64 [B][C][T]"""
    C, k, fam = c["C"], c["k"], c["fam"]
    a1, E1, _ = _pair_stage(c, lrelu32(inp["x"]), inp["w1"], c["dil"])
    v1 = a1 + inp["b1"].double().view(1, -1, 1)
    h = torch.where(v1 > 0, v1, v1 * float(np.float32(SLOPE)))
    e1 = E1 + U32 * (v1.abs() + h.abs())
    if fam == "bf16":
        e1, h = e1 + UB * (2 * h.abs() + e1), bf16r(h)
    elif fam == "x3":
        e1 = e1 + UB * UB * (h.abs() + e1)
    # the second stage on the reference intermediate; its operand is uncertain by e1
    w2 = inp["w2"]
    pad2 = (k - 1) // 2
    if fam == "mf":
        a2, E2, _, _ = _pair_stage_mf2(c, h, w2)
    else:
        wo = (sum(split(w2)) if fam == "x3" else bf16r(w2.double()) if fam == "bf16" else w2.double())
        a2 = F.conv1d(h, wo, padding=pad2)
        S2 = F.conv1d(h.abs() + e1, wo.abs(), padding=pad2)
        E2 = ((acc(3 * C * k) + UB * UB) if fam == "x3" else acc(C * k)) * S2
        E2 = E2 + F.conv1d(e1, wo.abs(), padding=pad2)
    if fam == "mf":      # (in exact arithmetic the pseudo-tap algebra IS the convolution, so e1 passes through it as through conv2 itself)
        E2 = E2 + F.conv1d(e1, w2.double().abs(), padding=pad2)
    return epilogue(a2, E2, inp["b2"], inp["x"], inp["out_in"], c["alpha"], c["beta"])


def _pair_stage_mf2(c, h, w2):
    a, E, plain, S, dis = mf_stage(h, w2, c["k"], 1, (c["k"] - 1) // 2, h.shape[-1], c["C"])
    c["mf_disagreement"] = max(c.get("mf_disagreement", 0.0), dis)
    return a, E, plain, S


def pair_emulation(c, inp):
    """the pair in float32 torch with the kernel's operand roundings -> fp32 [B][C][T]"""
    k, fam = c["k"], c["fam"]

    def conv(xin, w, dil):
        pad = (k - 1) * dil // 2
        if fam == "mf":
            A, _ = mf_accumulators(xin, pack.pack_conv_mf(w), k, dil, pad, xin.shape[-1], torch.float32)
            ye, yo, _, _ = mf_forms(A, torch.zeros_like(A), dil)
            return torch.where((torch.arange(xin.shape[-1]) // dil) % 2 == 0, ye, yo)
        if fam == "x3":
            (xh, xl), (wh, wl) = split(xin), split(w)
            xh, xl, wh, wl = xh.float(), xl.float(), wh.float(), wl.float()
            return F.conv1d(xl, wh, dilation=dil, padding=pad) + F.conv1d(xh, wl, dilation=dil, padding=pad) + F.conv1d(xh, wh, dilation=dil, padding=pad)
        if fam == "bf16":
            return F.conv1d(xin.bfloat16().float(), w.bfloat16().float(), dilation=dil, padding=pad)
        return F.conv1d(xin, w, dilation=dil, padding=pad)
    h = lrelu32(conv(lrelu32(inp["x"]), inp["w1"], c["dil"]) + inp["b1"].view(1, -1, 1))
    v = conv(h, inp["w2"], 1) + inp["b2"].view(1, -1, 1) + inp["x"]
    return v * np.float32(c["alpha"]) + (inp["out_in"] * np.float32(c["beta"]) if inp["out_in"] is not None else 0.0)


# ---- the cases of tests/test_gpu_conv_units.py (and of the host tests, which run the emulation and the plan query on every one) -----------------
def _cases():
    cs = []
    # CONV_F32, register-staged: channels that are no chunk of 16, Co % 4 != 0, halo 62 / 64 (behind the DMA kernels' 60), T around one MFMA column block
    for T in (1, 2, 63, 64, 65):
        cs.append(case("f32", 2, 20, T, 6, 3, 31, (F32, 32, 256)))
    cs += [case("f32", 2, 8, 65, 6, 3, 32, (F32, 32, 256)), case("f32", 3, 16, 64, 36, 5, 16, (F32, 64, 128), res=True),
           case("f32", 2, 16, 130, 68, 3, 32, (F32, 128, 128)), case("f32", 2, 20, 64, 64, 3, 1, (F32, 64, 128), T_out=62, pad=0),
           case("f32", 2, 20, 64, 64, 3, 1, (F32, 64, 128), T_out=66, pad=2), case("f32", 2, 16, 63, 64, 3, 1, (F32, 64, 128)),
           case("f32", 2, 16, 64, 32, 3, 1, (F32, 32, 256), mis=X_4B)]
    # CONV_F32G: the narrow builds and the 64 x 64 tile; (11, 6) = halo 60, the DMA limit; B = 3 x 3 time tiles = 9 units over 8 XCDs
    for Co, T, (k, dil) in ((4, 4, (1, 1)), (32, 60, (3, 1)), (36, 64, (7, 3)), (64, 68, (11, 5)), (64, 128, (11, 6)), (68, 132, (11, 6)),
                            (68, 64, (3, 1)), (132, 60, (7, 3))):
        cs.append(case("f32", 2, 16 if Co != 64 else 48, T, Co, k, dil, (F32G, 32 if Co <= 32 else 64, 256 if Co <= 32 else (128 if Co <= 64 else 64)),
                       res=Co in (36, 68)))
    cs += [case("f32", 3, 16, 132, 68, 3, 1, (F32G, 64, 64)), case("f32", 3, 16, 192, 128, 11, 6, (F32G, 64, 64), act=0),
           case("f32", 2, 16, 64, 64, 3, 1, (F32G, 64, 128), T_out=60, pad=0), case("f32", 2, 16, 64, 64, 3, 1, (F32G, 64, 128), T_out=66, pad=2),
           case("f32", 2, 16, 64, 64, 3, 1, (F32G, 64, 128), T_out=64, pad=1, mis=OUT_4B)]
    # CONV_F32G wide tiles: grids above 256 workgroups with a thin K; a full last time tile and one of 4 columns
    # (found with the plan query: the cheapest B, T, Co that g_pick_tile sends to each tile)
    cs += [case("f32", 11, 16, 96, 1536, 3, 1, (F32G, 128, 96)), case("f32", 11, 16, 196, 768, 3, 1, (F32G, 128, 96)),
           case("f32", 11, 16, 128, 1536, 3, 1, (F32G, 128, 128)), case("f32", 26, 16, 388, 256, 3, 1, (F32G, 128, 128)),
           case("f32", 11, 16, 128, 768, 3, 1, (F32G, 64, 128)), case("f32", 9, 16, 132, 768, 3, 1, (F32G, 64, 128)),
           case("f32", 9, 16, 68, 768, 3, 1, (F32G, 64, 64), res=True)]
    # conv1d_f32g's upsampled form (vb_conv1d_f32_ups): 4-byte window pieces, unaligned rows allowed; 96 and 128 wide
    for Co, T in ((128, 2), (132, 48), (128, 49), (132, 64), (128, 65)):
        cs.append(case("f32", 2, 16, T, Co, 3, 1, (F32G, 128, 96), ups=1, res=T == 48))
    cs.append(case("f32", 11, 16, 64, 1536, 3, 1, (F32G, 128, 128), ups=1))
    # transposed convolutions on the fp32 routes
    for (kt, u), T in (((4, 2), 1), ((4, 2), 19), ((16, 8), 2), ((16, 8), 19), ((15, 5), 2), ((15, 5), 19), ((11, 5), 1), ((11, 5), 19)):
        cs.append(case("f32", 2, 16, T, 32, 0, 1, (F32G if T % 4 == 0 else F32, 32, 256), tr=(u, kt)))
    cs.append(case("f32", 2, 16, 20, 68, 0, 1, (F32G, 64, 64), tr=(8, 16)))
    # T_out no multiple of u: the last phases have one output fewer
    cs += [case("f32", 2, 16, 19, 32, 0, 1, (F32, 32, 256), tr=(5, 11), T_out=94), case("f32", 2, 16, 20, 32, 0, 1, (F32G, 32, 256), tr=(5, 11), T_out=99),
           case("bf16", 2, 32, 19, 33, 0, 1, (BF16, 64, 128), tr=(8, 16), T_out=149)]
    cs += [case("f32", 2, 20, 19, 6, 0, 1, (F32, 32, 256), tr=(5, 11)), case("x3", 2, 32, 19, 64, 0, 1, (X3, 64, 128), tr=(8, 16))]
    # CONV_CO1
    for Ci, T, k in ((16, 1, 7), (80, 255, 7), (16, 256, 1), (80, 257, 7), (16, 513, 7)):
        cs.append(case("f32", 2, Ci, T, 1, k, 1, (CO1, 1, 512)))
    # CONV_F32W: every kernel size at both ends of the dilation range inside halo <= 60; T around the tile
    for k, dil, Co, Ci, T in ((3, 1, 32, 16, 4), (3, 8, 36, 48, 8), (5, 1, 128, 16, 124), (5, 8, 132, 16, 128), (7, 1, 32, 48, 252), (7, 8, 128, 16, 132),
                              (11, 1, 36, 16, 256), (11, 6, 128, 16, 260), (11, 5, 132, 48, 120), (7, 3, 64, 16, 244)):
        for (al, be, rs) in (((1.0, 0.0, False), (1.0 / 3, 1.0, True)) if k in (3, 11) else ((1.0 / 3, 1.0, k == 7),)):
            vw = 32 // dil * dil
            narrow = Co <= 64 or 0 < Co % 128 <= 64
            cs.append(case("mf", 3 if T > 100 else 2, Ci, T, Co, k, dil, (F32W, 64 if narrow else 128, (8 if narrow else 4) * vw), alpha=al, beta=be, res=rs))
    # CONV_X3 / CONV_BF16: the four staged tiles, Ci < Ci_pad, strided input, upsampling
    for fam, rt in (("x3", X3), ("bf16", BF16)):
        for Co, T, Ci in ((8, 255, 20), (32, 257, 32), (33, 127, 48), (64, 129, 20), (65, 63, 32), (128, 65, 48), (132, 129, 20)):
            tile = (32, 256) if Co <= 32 else (64, 128) if Co <= 64 else (128, 64)
            cs.append(case(fam, 2, Ci, T, Co, 3, 2, (rt, *tile), res=Co in (33, 132)))
        cs.append(case(fam, 15, 32, 132, 1536, 3, 1, (rt, 128, 128), act=0))      # (180 of 256 workgroup slots: the smallest grid conv_staged_tile gives the big tile)
        cs.append(case(fam, 2, 20, 33, 65, 5, 1, (rt, 128, 64), T_out=33, pad=2))
    for ph, T in ((0, 33), (1, 33), (0, 34), (1, 34)):
        cs.append(case("bf16", 2, 20, T, 33, 3, 1, (BF16, 64, 128), stride=2, phase=ph, pad=1))
    cs += [case("bf16", 2, 32, 33, 65, 3, 1, (BF16, 128, 64), ups=1), case("bf16", 2, 32, 64, 64, 3, 1, (BF16, 64, 128), alpha=1.0 / 3, beta=1.0, res=True)]
    # bf16xt: the one-plane GEMM route and conv1d_bf16_kernel's DMA-fed input mode
    for Co, T, pad in ((384, 1, 1), (388, 63, 1), (384, 64, 1), (388, 65, 1), (384, 129, 1)):
        cs.append(case("bf16xt", 2, 64, T, Co, 3, 1, (AS_GEMM, 64, 64), pad=pad, res=Co == 388))
    cs += [case("bf16xt", 2, 64, 65, 384, 3, 1, (BF16_XT, 128, 64), knobs={"VB_CONV_GEMM_OFF": "1"}),
           case("bf16xt", 2, 64, 64, 384, 1, 1, (BF16_XT, 128, 64), pad=0, alpha=1.0 / 3, beta=1.0),
           case("bf16xt", 2, 64, 63, 132, 3, 1, (BF16_XT, 128, 64), T_out=65, pad=2),
           case("bf16xt", 2, 64, 64, 388, 3, 32, (BF16_XT, 128, 64), T_out=64 + 2 * 64 - 64, pad=64)]
    # the same two routes in the split precision (vb_conv1d_x3_xt): three-pass GEMM and conv1d_x3_kernel's DMA-fed input mode
    for Co, T in ((384, 1), (388, 63), (384, 64), (388, 65), (384, 129)):
        cs.append(case("x3xt", 2, 64, T, Co, 3, 1, (AS_GEMM, 64, 64), res=Co == 388))
    cs += [case("x3xt", 2, 64, 65, 384, 3, 1, (X3_XT, 128, 64), knobs={"VB_CONV_GEMM_OFF": "1"}),
           case("x3xt", 2, 64, 64, 384, 1, 1, (X3_XT, 128, 64), pad=0, alpha=1.0 / 3, beta=1.0),
           case("x3xt", 2, 64, 63, 132, 3, 1, (X3_XT, 128, 64), T_out=65, pad=2),
           case("x3xt", 2, 64, 64, 388, 3, 32, (X3_XT, 128, 64), T_out=128, pad=64), case("x3xt", 2, 64, 33, 132, 3, 1, (X3_XT, 128, 64), ups=1)]
    # GroupNorm and GroupNorm + swish, one and four channels per group, on the one-plane kernel, its DMA-fed mode and the GEMM route
    for swish in (0, 1):
        cs += [case("bf16", 2, 32, 65, 33, 3, 1, (BF16, 64, 128), gn=(32, swish)), case("bf16", 2, 32, 37, 65, 3, 1, (BF16, 128, 64), gn=(8, swish)),
               case("bf16xt", 2, 64, 65, 132, 3, 1, (BF16_XT, 128, 64), gn=(64, swish)), case("bf16xt", 2, 64, 64, 132, 3, 1, (BF16_XT, 128, 64), gn=(16, swish)),
               case("bf16xt", 2, 64, 65, 384, 3, 1, (AS_GEMM, 64, 64), gn=(16 if swish else 64, swish))]
    # operands that are only 4-byte aligned, on the routes that take them (register-staged windows, the direct epilogue)
    cs += [case("x3", 2, 20, 65, 33, 3, 1, (X3, 64, 128), res=True, mis=X_4B | OUT_4B | RES_4B), case("bf16", 2, 20, 64, 65, 3, 1, (BF16, 128, 64), res=True, mis=X_4B | OUT_4B | RES_4B),
           case("f32", 2, 20, 64, 36, 3, 1, (F32, 64, 128), res=True, mis=RES_4B), case("f32", 2, 16, 19, 32, 0, 1, (F32, 32, 256), tr=(2, 4), mis=X_4B | OUT_4B),
           case("bf16", 2, 32, 19, 33, 0, 1, (BF16, 64, 128), tr=(5, 15), mis=X_4B | OUT_4B)]
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


def _pair_cases():
    ps = []
    for form in (PAIR_F32, PAIR_MF, PAIR_X3, PAIR_BF16):
        Ts = (4, 124, 128, 132, 256) if form in (PAIR_F32, PAIR_MF) else (1, 4, 124, 128, 132, 256)
        kd = ((3, 1), (7, 3), (11, 5))
        Cs = (32, 64, 128) if form == PAIR_F32 else (32, 64)
        for i, T in enumerate(Ts):
            k, dil = kd[i % 3]
            ps.append(pair_case(form, 3, Cs[i % len(Cs)], T, k, dil, *((1.0, 0.0) if i % 2 == 0 else (1.0 / 3, 1.0))))
    return ps


CASES = _cases()
PAIR_CASES = _pair_cases()


# ---- the plan queries (host only) ------------------------------------------------------------------------------------------------------------
def conv_plan(lib, c):
    """(route, tile_co, tile_t, stage_epi) of the call as the library would run it now"""
    import ctypes as C
    r = [C.c_int() for _ in range(4)]
    rc = lib.vb_conv1d_plan(c["B"], c["Ci"], c["T"], c["Co"], c["k"], c["dil"], c["pad"], c["u"], c["tr_pad"], c["tr_k"], c["T_out"], c["ups"],
                            c["stride"], c["phase"], c["act"], c["gn"][0] if c["gn"] else 32, c["alpha"], c["beta"], c["wforms"], c["Ci_pad"],
                            c["xt"], int(c["res"]), c["mis"], *[C.byref(v) for v in r])
    assert rc == 0, (c["id"], lib.vb_last_error())
    return tuple(v.value for v in r)


def pair_plan(lib, c):
    """(run, outputs per workgroup, workgroups along time, staged epilogue)"""
    import ctypes as C
    r = [C.c_int() for _ in range(4)]
    rc = lib.vb_respair_plan(c["form"], c["B"], c["C"], c["T"], c["k"], c["dil"], 0, *[C.byref(v) for v in r])
    assert rc == 0, (c["id"], lib.vb_last_error())
    return tuple(v.value for v in r)


def assert_plan(lib, c):
    """the case still reaches the kernel and tile it was written for (None = that component is not pinned)"""
    got = conv_plan(lib, c)
    want = c["plan"]
    assert all(w is None or w == g for w, g in zip(want, got)), f"{c['id']}: planned as {got}, written for {want}"
    return got
