"""Float64 row oracles of the attention half's two launches - attn_kernel (vb_attention / vb_attention_lens) and the QKV GEMM with the
RoPE / V-transpose epilogue (vb_qkv_rope) - each with a derived per-element error bound (plain torch, CPU), in the style of
tests/moe_oracles.py, whose constants U32, UB, acc() and bf16r() are used here.  Both oracles are evaluated on the plane values the
kernels read: bf16 for np = 1, hi + lo for np = 2 ("split": every product is hi*hi + lo*hi + hi*lo, three exact fp32 products per term,
nseg = 3; the lo*lo product is dropped).  All bounds are first order in U32 / UB, like those of moe_oracles.

attention(q, k, v, ky, vy, cross_w, lens, np):  ref = softmax(q k^T / sqrt(hd)) v + cross_w[h] * softmax(q ky^T / sqrt(hd)) vy - two SEPARATE
softmaxes; with lens row b attends over its first lens[b] keys and only its query rows < lens[b] are defined (NaN elsewhere).

One pass over S keys (P = the normalised softmax, out = P v, c = log2(e) / sqrt(hd), a_j = c s_j, M = max_j a_j), as attn_kernel runs it:
  Score.  s_j = q . k_j accumulates hd * nseg exact products:  es_j = acc(hd nseg) (|q| . |k_j|)  [+ UB^2 (|q| . |k_j|), np = 2: the
    dropped lo*lo product].  The kernel forms p_j = exp2(fma(s_j, c32, -m)) with m the row's running maximum, the SAME m in numerator and
    row sum (a rescale multiplies both by the same alpha, so neither m nor alpha's own error reaches the quotient).  Its exponent is off
    by  c es_j  +  4 U32 |a_j|  (c32 = fl(fl(1 / sqrtf(hd)) * log2e): four roundings)  +  U32 (M - a_j + THR + 1)  (the fma's one rounding;
    its result is at most THR = 8, the default VB_ATTN_DEFER, above zero and at most M - a_j below), and v_exp_f32 adds 2 U32:
        eps_j = ln2 (c es_j + 4 U32 |a_j| + U32 (M - a_j + 9)) + 2 U32        relative, on p_j.
    (A p_j below 2^-126 is flushed to zero: an absolute 1e-38, not counted.)
  Exponent error in numerator and denominator.  The simple form is eps_max ((P|v|)[d] + |out[d]|); the kernel's error is per key, so the
    tighter and still rigorous  sum_j P_j eps_j |v_j[d]|  +  |out[d]| sum_j P_j eps_j  is used: a planted key with a long k row has a
    large es_j but also carries its own weight, it does not tax the other keys.
  P rounding.  The row sum adds the unrounded fp32 p; the product takes bf16(p) (np = 1): UB (P|v|)[d]; or hi + lo of p against v's
    hi + lo WITHOUT the lo*lo product (np = 2): 2 UB^2 (P|v|)[d] - UB^2 for p's own hi + lo, UB^2 more because the kernel drops p_lo v_lo as it drops q_lo k_lo.
    Independent of VB_ATTN_DEFER: a deferred maximum scales p by at most 2^THR before a RELATIVE rounding.
  Accumulation.  acc(64 ntiles nseg) (P|v|)[d] for the accumulator (masked keys enter as exact zeros: p = 0 times a finite pad), the same
    with nseg = 1 times |out[d]| for the fp32 row sum, and one U32 on each per rescale, at most ntiles = ceil(S / 64) of them.
  Normalisation.  Two roundings (reciprocal or quotient, product): 2 U32 |out[d]|.
Cross scales by |cross_w[h]| (its quotient and product are the two normalisation roundings); the self pass's product and the stash add
are at most two more roundings of the sum: 2 U32 (|self| + |w cross|).  With E the sum of all this the one output rounding gives
    bound = E + u (|ref| + E),    u = UB (np = 1),  UB^2 (np = 2: hi + lo).

qkv_rope(u, wqkv, cos, sin, B, T, H, hd, np):  y = u Wqkv^T  with  ey = acc(K nseg) |u| |W|^T [+ UB^2 |u| |W|^T];  the q and k thirds rotate
the pair (v0, v1) = y[2j], y[2j + 1] of every head by (c, s) = (cos, sin)[t][j] as epi_store<EPI_QKV_ROPE> writes it,
    o0 = fma(v0, c, -(v1 s)),  o1 = fma(v0, s, v1 c):    E = e0 |c| + e1 |s| + 2 U32 (|v0 c| + |v1 s|)   (o1: c and s exchanged),
the V third is y itself at vt[b][h][d][t] (E = ey).  Plane stores round BOTH sides (moe_oracles' rule): ref = the planes of the float64
value, bound = E + u (2 |x| + E)."""
from __future__ import annotations

import functools
import math

import torch

from tests.moe_oracles import U32, UB, acc, bf16r, rnd, worst   # noqa: F401  (worst: re-exported for the tests)
from versband_amd import pack

HD = 96
KT = 64                  # keys per tile of attn_kernel
THR = 8.0                # default VB_ATTN_DEFER (log2 units)
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
BIG = 2.0 ** 14          # what V^T pad columns hold in the GPU tests: finite, and thousands of times any bound if it leaks


def plane_values(x: torch.Tensor, np_: int) -> torch.Tensor:
    """fp32 -> what a kernel reads from the bf16 planes of x, as float64"""
    return pack.to_planes(x, np_).double().sum(0)


def planes_r(x: torch.Tensor, np_: int) -> torch.Tensor:
    """float64 -> the value its planes hold (np = 1: nearest bf16; np = 2: hi + lo), float64"""
    hi = bf16r(x)
    return hi if np_ == 1 else hi + bf16r(x - hi)


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_pass(q, k, v, np_):
    """q [.., T, hd], k / v [.., S, hd] float64 plane values -> (out, E, P) of one normalised pass, E before any output rounding"""
    hd, S = q.shape[-1], k.shape[-2]
    nseg = 1 if np_ == 1 else 3
    c = LOG2E / math.sqrt(hd)
    s, sa = q @ k.transpose(-1, -2), q.abs() @ k.abs().transpose(-1, -2)
    es = (acc(hd * nseg) + (UB * UB if np_ == 2 else 0.0)) * sa
    a = s * c
    eps = LN2 * (c * es + 4 * U32 * a.abs() + U32 * (a.amax(-1, keepdim=True) - a + THR + 1)) + 2 * U32
    P = torch.softmax(s / math.sqrt(hd), -1)
    out, PV, Pe = P @ v, P @ v.abs(), P * eps
    ntiles = (S + KT - 1) // KT
    prnd = UB if np_ == 1 else 2 * UB * UB
    E = (Pe @ v.abs() + out.abs() * Pe.sum(-1, keepdim=True) + (prnd + acc(KT * ntiles * nseg) + ntiles * U32) * PV +
         (acc(KT * ntiles) + ntiles * U32 + 2 * U32) * out.abs())
    return out, E, P


def attention(q, k, v, ky, vy, cross_w, lens=None, np=1, key_lens=None):
    """q [B][T][H][hd]; k, v [B][S][H][hd] (None: no self pass); ky, vy [B][Lc][H][hd] (None: no cross pass); cross_w [H] or None (weight 1)
    - float64 plane values -> (ref, bound) float64 [B][T][H][hd]; rows >= lens[b] are NaN in both.  key_lens (the host test's wrong results
    only): the self pass's key count of every row where it is not lens[b] / S."""
    B, T, H, _ = q.shape
    hm = lambda x: x.permute(0, 2, 1, 3)                                 # -> [B][H][.][hd]
    ref = torch.zeros(B, H, T, q.shape[-1], dtype=torch.float64)
    E = torch.zeros_like(ref)
    if ky is not None:
        w = (cross_w.double() if cross_w is not None else torch.ones(H, dtype=torch.float64)).view(1, H, 1, 1)
        o, e, _ = softmax_pass(hm(q), hm(ky), hm(vy), np)
        ref, E = w * o, w.abs() * e
    if k is not None:
        cross = ref.clone()
        for b in range(B):
            n = T if lens is None else int(lens[b])
            nk = int(key_lens[b]) if key_lens is not None else (k.shape[1] if lens is None else n)
            o, e, _ = softmax_pass(hm(q)[b, :, :n], hm(k)[b, :, :nk], hm(v)[b, :, :nk], np)
            ref[b, :, :n] += o
            E[b, :, :n] += e + 2 * U32 * (o.abs() + cross[b, :, :n].abs())
            ref[b, :, n:], E[b, :, n:] = float("nan"), float("nan")
    u = UB if np == 1 else UB * UB
    return hm(ref).contiguous(), hm(E + u * (ref.abs() + E)).contiguous()


def dominant_pass(q, k, v, ky, vy, cross_w, idx, np=1):
    """which pass carries the reference at element idx = (b, t, h, d): for failure reports"""
    b, t, h, d = idx
    parts = {}
    if k is not None:
        parts["self"] = abs(float(attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], None, None, None, None, np)[0][0, t, h, d]))
    if ky is not None:
        parts["cross"] = abs(float(attention(q[b:b + 1], None, None, ky[b:b + 1], vy[b:b + 1], cross_w, None, np)[0][0, t, h, d]))
    return max(parts, key=lambda n: parts[n] if parts[n] == parts[n] else -1.0)


def boundary_keys(n):
    """the keys whose loss or gain a tile-edge bug shows as: first, both sides of the 64-key seam, last"""
    return sorted({j for j in (0, KT - 1, KT, n - 1) if 0 <= j < n})


def planted_rows(n_rows, n_keys, cross):
    """the query row r_j of every boundary key j: spread over the rows, the last key on the last row (self) / the one before it (cross)"""
    ks = boundary_keys(n_keys)
    lo, hi = (1, n_rows - 2) if cross and n_rows >= 2 * len(ks) + 2 else (0, n_rows - 1)
    return {j: lo + (i * (hi - lo)) // max(len(ks) - 1, 1) if len(ks) > 1 else hi for i, j in enumerate(ks)}


def quiet_row(n_rows, n_cross_keys):
    """the query row scaled down to scores near zero, where a leaked pad key of score 0 weighs as much as any real key (a row whose
    maximum lies ten units above zero would hide it): the first row from the middle on that no boundary key is planted on; None if all are"""
    taken = set(planted_rows(n_rows, n_rows, False).values()) | set(planted_rows(n_rows, n_cross_keys, True).values())
    return next((r for r in range(n_rows // 2, n_rows) if r not in taken), None)


def plant(q, k, n_rows, n_keys, cross):
    """k[j] parallel to q[r_j] for every boundary key j, with the gain at which that key carries half of row r_j's softmax (q [T][H][hd] and
    k [S][H][hd] of one batch row, k modified in place; computed on the fp32 values - the plane rounding moves the share by a few percent)"""
    rows = planted_rows(n_rows, n_keys, cross)
    for j, r in rows.items():
        qr = q[r].double()                                                  # [H][hd]
        s = torch.einsum("hd,shd->hs", qr, k[:n_keys].double()) / math.sqrt(HD)
        s[:, [i for i in rows if rows[i] == r]] = -float("inf")             # (planted keys that share a row share its softmax equally)
        lse = torch.logsumexp(s, 1).clamp(min=0.0)                          # (no other key: the planted ones are all there is)
        gain = lse.clamp(min=1.0) * math.sqrt(HD) / qr.pow(2).sum(1)        # q_r . k_j / sqrt(hd) = max(lse, 1) of the other keys
        k[j] = (qr * gain.unsqueeze(1)).float()


@functools.lru_cache(maxsize=None)
def attn_case(B, H, T, Lc, lens=None):
    """The inputs of the GPU tests and of the host test (fp32, before the plane rounding).  q is scaled by 3: scores of standard deviation
    ~3, not 1 - a flat softmax over hundreds of keys is where UB (P|v|) swallows one key.  Boundary keys are planted (plant()) and one query
    row per batch row is quiet (quiet_row()).  With lens,
    q / k rows and v rows >= lens[b] hold large finite values: 64 x noise in q and k, BIG in v."""
    tag = f"at{B}_{H}_{T}_{Lc}" + ("l" if lens else "")
    sh, shy = (B, T, H, HD), (B, Lc, H, HD)
    c = dict(B=B, H=H, T=T, Lc=Lc, lens=lens, q=rnd(sh, tag + "q", 3.0).float(), k=rnd(sh, tag + "k").float(), v=rnd(sh, tag + "v").float(),
             ky=rnd(shy, tag + "ky").float(), vy=rnd(shy, tag + "vy").float(), cw=rnd((H,), tag + "cw").float())
    for b in range(B):
        n = T if lens is None else lens[b]
        plant(c["q"][b], c["k"][b], n, n, False)
        plant(c["q"][b], c["ky"][b], n, Lc, True)
        if quiet_row(n, Lc) is not None:
            c["q"][b, quiet_row(n, Lc)] /= 64.0
        if n < T:
            c["q"][b, n:] *= 64.0 / 3.0
            c["k"][b, n:] *= 64.0
            c["v"][b, n:] = BIG
    return c


@functools.lru_cache(maxsize=None)
def attn_reference(B, H, T, Lc, lens, np_, use_self, use_cross):
    c = attn_case(B, H, T, Lc, lens)
    pv = {n: plane_values(c[n], np_) for n in ("q", "k", "v", "ky", "vy")}
    return attention(pv["q"], pv["k"] if use_self else None, pv["v"] if use_self else None, pv["ky"] if use_cross else None,
                     pv["vy"] if use_cross else None, c["cw"] if use_cross else None, lens, np_)


PLAIN_CASES = [(1, 1, 1, 1), (1, 2, 33, 64), (1, 1, 64, 65), (2, 2, 65, 80), (1, 1, 128, 1), (3, 3, 129, 16), (1, 8, 129, 65)]     # (B, H, T, Lc)
MODES = [(False, True), (True, False), (True, True)]                     # (self, cross)
DEFER_CASE = (3, 3, 129, 16)
LENS_T, LENS_H, LENS_LC, LENS = 130, 2, 16, (130, 129, 128, 65, 64, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# QKV projection + RoPE + V transpose
# ---------------------------------------------------------------------------------------------------------------------------------
def qkv_rope(u, wqkv, cos, sin, B, T, H, hd, np):
    """u [B*T][D], wqkv [3D][D] float64 plane values, cos / sin [>= T][hd / 2] -> (q, k, vt, bq, bk, bvt): q, k [B*T][D], vt [B][H][hd][T]"""
    D, M = H * hd, B * T
    nseg = 1 if np == 1 else 3
    y = u @ wqkv.T
    ey = (acc(D * nseg) + (UB * UB if np == 2 else 0.0)) * (u.abs() @ wqkv.abs().T)
    t = torch.arange(M) % T
    c = cos.double()[t].repeat(1, H)                                     # [M][D / 2]: pair j of head h at column h * hd / 2 + j
    s = sin.double()[t].repeat(1, H)
    uu = UB if np == 1 else UB * UB
    outs, bounds = [], []
    for sec in range(2):
        v0, v1 = y[:, sec * D:(sec + 1) * D:2], y[:, sec * D + 1:(sec + 1) * D:2]
        e0, e1 = ey[:, sec * D:(sec + 1) * D:2], ey[:, sec * D + 1:(sec + 1) * D:2]
        x = torch.stack([v0 * c - v1 * s, v0 * s + v1 * c], 2).reshape(M, D)
        E = torch.stack([e0 * c.abs() + e1 * s.abs() + 2 * U32 * ((v0 * c).abs() + (v1 * s).abs()),
                         e0 * s.abs() + e1 * c.abs() + 2 * U32 * ((v0 * s).abs() + (v1 * c).abs())], 2).reshape(M, D)
        outs.append(planes_r(x, np))
        bounds.append(E + uu * (2 * x.abs() + E))
    tr = lambda x: x.view(B, T, H, hd).permute(0, 2, 3, 1).contiguous()
    yv, ev = y[:, 2 * D:], ey[:, 2 * D:]
    return outs[0], outs[1], tr(planes_r(yv, np)), bounds[0], bounds[1], tr(ev + uu * (2 * yv.abs() + ev))


QKV_H = 2
QKV_CASES = [(3, 65, 128), (2, 64, 64), (3, 129, 192), (1, 1, 64)]       # (B, T, Tpad)
QKV_P8_T = 130


def p8_min_clips(T=QKV_P8_T, H=QKV_H):
    """the smallest B at which the QKV launch makes P8_MIN_TILES (gemm_bf16.hip) 256 x 256 tiles: the 8-wave kernel's threshold"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "versband_amd", "csrc", "gemm_bf16.hip")).read()
    need = int(re.search(r"#define\s+P8_MIN_TILES\s+(\d+)", src).group(1))
    ncol = (3 * H * HD + 255) // 256
    B = 1
    while (B * T + 255) // 256 * ncol < need:
        B += 1
    return B


@functools.lru_cache(maxsize=None)
def qkv_case(B, T, H=QKV_H):
    """u ~ N(0, 1), W ~ N(0, 1 / D); cos / sin uniform in [-1, 1] and independent - no rotation, so exchanged tables or a wrong sign show.
    The tables hold one row more than T: the mutation "t of the wrong clip" of the host test reads it, the kernel must not."""
    D = H * HD
    tag = f"qr{B}_{T}_{H}"
    uni = lambda name: torch.erf(rnd((T + 1, HD // 2), tag + name) / math.sqrt(2.0)).float()
    return dict(B=B, T=T, H=H, u=rnd((B * T, D), tag + "u").float(), w=rnd((3 * D, D), tag + "w", D ** -0.5).float(), cos=uni("c"), sin=uni("s"))


@functools.lru_cache(maxsize=None)
def qkv_reference(B, T, np_, H=QKV_H):
    c = qkv_case(B, T, H)
    return qkv_rope(plane_values(c["u"], np_), plane_values(c["w"], np_), c["cos"][:T], c["sin"][:T], B, T, H, HD, np_)
