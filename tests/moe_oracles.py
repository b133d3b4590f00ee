"""Float64 oracles of the MoE block's fused kernels, stage by stage, each with a derived per-element error bound (plain torch, CPU).

Every stage is evaluated in float64 on that stage's own bf16 / fp32 inputs, so only one stage's rounding is in play and its bound can be
written down instead of guessed.  Constants (all bounds are first order in them):

  U32 = 2^-24   unit roundoff of fp32: one round-to-nearest operation errs by at most U32 |result|.
  UB  = 2^-8    unit roundoff of bf16 (8 significant bits): |bf16(x) - x| <= UB |x|, neighbouring bf16 values are at most 2 UB |x| apart.
  acc(K) = 2 K U32   fp32 accumulation of K exact products (a bf16 x bf16 product has 16 significant bits: exact in fp32) in ANY order:
      one rounding per addition gives (K - 1) U32 sum|x_k w_k|; the factor 2 covers an adder tree inside the matrix instruction that
      need not round to nearest at every step.  The bound is relative to sum |x_k| |w_k|, not to the result: cancellation is covered.
  silu: x / (1 + exp(-x)) with a fast exponential (argument scaled to base 2: (|x| + 2) U32) and a 1-ulp reciprocal - at most
      (|x| + 8) U32 relative with the add and the two multiplications; |silu'| <= 1.1 everywhere.

Where a device value and the reference are both ROUNDED to bf16 from values E apart, they differ by at most E + UB (|x_dev| + |x_ref|)
<= E + UB (2 |x_ref| + E): equal, or on neighbouring bf16 values ("one bf16 ulp", 2 UB |x| at its largest)."""
from __future__ import annotations

import math

import numpy as np
import torch

from versband_amd import prng

U32 = 2.0 ** -24
UB = 2.0 ** -8


def acc(K: int) -> float:
    return 2.0 * K * U32


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """float64 -> nearest bf16, as float64 (through fp32: the double rounding moves a value only when float64 sits within 2^-29 of a
    bf16 tie, which every bound here covers as a neighbouring-value case)"""
    return x.float().bfloat16().double()


def silu64(a: torch.Tensor) -> torch.Tensor:
    return a * torch.sigmoid(a)


def rnd(shape, name, scale=1.0) -> torch.Tensor:
    n = int(np.prod(shape))
    return torch.from_numpy(prng.normal(prng.key_seed(11, name), n).reshape(shape)) * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# band-expert FFN:  out[m][e band + n] = out_in + gate[m // T][e band + n] * (h W2_e^T)[n],  h = bf16(silu(y_e W1_e^T) * (y_e W3_e^T))
# ---------------------------------------------------------------------------------------------------------------------------------
def band_ffn(y, w13, w2, gate, out_in, T, E, band):
    """y [M][>= E band] bf16 values, w13 [E][2H][band] (w1 / w3 rows interleaved), w2 [E][band][H], gate [>= ceil(M / T)][>= E band] fp32,
    out_in [M][>= E band] fp32  ->  (ref, bound), float64 [M][E band].

    The hidden value never leaves the kernel, so both products are one stage.  The fp32 error of the first product and of silu (~2^-20
    relative) reaches the output only where it moves a hidden value across a bf16 rounding boundary, onto the neighbouring bf16:
        bound = |gate| (UB S + acc(H) S) + U32 (|out_in| + |gate| |z|),    z = h W2^T,  S = |h| |W2|^T
    UB S: every hidden value of the row off by half the largest bf16 spacing at once - such crossings are rare (the fp32 error over the
    bf16 spacing, ~2^-12 of the values), a single one costs 2 UB |h_k w_k|, far below UB S for the 64 and more terms summed here;
    acc(H) S: fp32 accumulation of the second product; the last term: the one rounding of the fused multiply-add that updates out."""
    M, H, D = y.shape[0], w2.shape[2], E * band
    clip = torch.arange(M) // T
    ref = torch.empty(M, D, dtype=torch.float64)
    bound = torch.empty(M, D, dtype=torch.float64)
    for e in range(E):
        cols = slice(e * band, (e + 1) * band)
        ye = y[:, cols].double()
        a, b = ye @ w13[e, 0::2].double().T, ye @ w13[e, 1::2].double().T
        h = bf16r(silu64(a) * b)
        W2 = w2[e].double()
        z, S = h @ W2.T, h.abs() @ W2.abs().T
        g, o = gate[clip][:, cols].double(), out_in[:, cols].double()
        ref[:, cols] = o + g * z
        bound[:, cols] = g.abs() * (UB + acc(H)) * S + U32 * (o.abs() + g.abs() * z.abs())
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# routed experts, first stage: hidden[slot] = bf16(m * silu(u W1_g^T) * (u W3_g^T)),  u = u[perm[slot]],  m = mc[tok] (slot < N) / ma[tok]
# ---------------------------------------------------------------------------------------------------------------------------------
def swiglu_folded(u, perm, group_off, w13, mc, ma, N):
    """u [N][D] bf16 values, perm [>= 2N] / group_off [G + 1] as the bucket kernel wrote them, w13 [G][2H][D] interleaved, mc / ma [N] fp32
    -> (ref, bound) float64 [2N][H] in slot order.

    a, b carry ea = acc(D) |u| |W1|^T, eb likewise; x = m silu(a) b is then off by at most
        E = |m| (1.1 ea |b| + |silu(a)| eb + 1.1 ea eb) + (|a| + 11) U32 |x|        (silu: (|a| + 8) U32, three more roundings)
    and both sides round to bf16:  bound = E + UB (2 |x| + E)."""
    G, H, D = w13.shape[0], w13.shape[1] // 2, u.shape[1]
    ref = torch.zeros(2 * N, H, dtype=torch.float64)
    bound = torch.zeros(2 * N, H, dtype=torch.float64)
    off = [int(v) for v in group_off]
    for g in range(G):
        slots = torch.arange(off[g], off[g + 1])
        if not slots.numel():
            continue
        tok = perm[slots].long()
        x = u[tok].double()
        W1, W3 = w13[g, 0::2].double(), w13[g, 1::2].double()
        a, b = x @ W1.T, x @ W3.T
        ea, eb = acc(D) * (x.abs() @ W1.abs().T), acc(D) * (x.abs() @ W3.abs().T)
        m = torch.where(slots < N, mc[tok], ma[tok]).double().unsqueeze(1)
        s = silu64(a)
        pre = m * s * b
        epre = m.abs() * (1.1 * ea * b.abs() + s.abs() * eb + 1.1 * ea * eb) + (a.abs() + 11.0) * U32 * pre.abs()
        ref[slots] = bf16r(pre)
        bound[slots] = epre + UB * (2 * pre.abs() + epre)
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# routed experts, second stage: out[perm[p]] = bf16(Hs[p] W2[c]^T + Hs[pair_pa[p]] W2[E + a]^T),  p in pair bucket (c, a)
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_w2(hs, w2, perm, pair_off, pair_pa, N, E):
    """hs [2N][H] the hidden values the device wrote (bf16), w2 [2E][D][H] -> (ref, bound) float64 [N][D] by token; rows of tokens in no
    bucket stay NaN.  One accumulator over K = 2H exact products, then one bf16 rounding on both sides:
        Ea = acc(2H) (|Hs[p]| |W2c|^T + |Hs[pa]| |W2a|^T),   bound = Ea + UB (2 |x| + Ea)      (one bf16 ulp of the result at its largest)"""
    D, H = w2.shape[1], w2.shape[2]
    ref = torch.full((N, D), float("nan"), dtype=torch.float64)
    bound = torch.full((N, D), float("nan"), dtype=torch.float64)
    off = [int(v) for v in pair_off]
    for g in range(E * E):
        c, a = divmod(g, E)
        p = torch.arange(off[g], off[g + 1])
        if not p.numel():
            continue
        tok = perm[p].long()
        A, Bm = hs[p].double(), hs[pair_pa[p].long()].double()
        Wc, Wa = w2[c].double(), w2[E + a].double()
        x = A @ Wc.T + Bm @ Wa.T
        ea = acc(2 * H) * (A.abs() @ Wc.abs().T + Bm.abs() @ Wa.abs().T)
        ref[tok] = bf16r(x)
        bound[tok] = ea + UB * (2 * x.abs() + ea)
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# caption gate: scores -> per-head softmax over the keys -> contraction with VW -> + bg; routing decisions
# ---------------------------------------------------------------------------------------------------------------------------------
def caption_logits(x, keys, sbias, vw, bg, T, Hh):
    """x [N][K] bf16 values (row n of clip n // T), keys [Beff][NS][K] bf16 values, sbias [Beff][NS], vw [Beff][NS][E], bg [E] (fp32)
    -> (lc, bound) float64 [N][E]: lc = logit + bg, score column = key * Hh + head.

    es = (acc(K) + U32) (|x| |keys|^T + |sbias|): a score and its bias add.  A probability p = exp(s - m) moves by exp(2 es) - 1 through
    its score and the maximum, and by (r + 4) 2 U32 through the fast exponential (r = the largest m - s of the row: rounding of the
    difference, of its scaling to base 2, 1 ulp of the instruction); normalising doubles that and adds the sum over L keys and the
    reciprocal:   rho = 2 (exp(2 max es) - 1 + (r + 4) 2 U32) + (L + 2) U32     relative, on every normalised probability q.
    The contraction over NS terms adds (NS + 4) U32 (products are rounded here, q and VW are fp32), the bias one more rounding:
        bound = (rho + (NS + 4) U32) q |VW| + U32 (|lc| + |bg|)."""
    N, K = x.shape
    Beff, NS, _ = keys.shape
    E, L = vw.shape[2], NS // Hh
    clip = torch.arange(N) // T
    s = torch.empty(N, NS, dtype=torch.float64)
    sa = torch.empty(N, NS, dtype=torch.float64)
    for b in range(Beff):
        rows = clip == b
        xb, kb = x[rows].double(), keys[b].double()
        s[rows] = xb @ kb.T + sbias[b].double()
        sa[rows] = xb.abs() @ kb.abs().T + sbias[b].double().abs()
    es = (acc(K) + U32) * sa
    s3 = s.view(N, L, Hh)
    m = s3.max(1, keepdim=True).values
    q = torch.softmax(s3, 1)
    vwn = vw.double()[clip].view(N, L, Hh, E)
    logit = torch.einsum("nlh,nlhe->ne", q, vwn)
    A = torch.einsum("nlh,nlhe->ne", q, vwn.abs())
    lc = logit + bg.double()
    r = (m - s3).amax((1, 2))
    rho = 2 * (torch.expm1(2 * es.amax(1)) + (r + 4) * 2 * U32) + (L + 2) * U32
    bound = (rho.unsqueeze(1) + (NS + 4) * U32) * A + U32 * (lc.abs() + bg.double().abs())
    return lc, bound


def first_argmax(z):
    """index of the first maximum of every row (torch.argmax returns the first of equal maxima)"""
    return z.argmax(1)


def margin(z):
    """top-1 minus top-2 of every row (infinite for a single column)"""
    if z.shape[1] < 2:
        return torch.full((z.shape[0],), float("inf"), dtype=z.dtype)
    t = z.topk(2, 1).values
    return t[:, 0] - t[:, 1]


def routing(lc, lc_bound, la_rows, g2, g3):
    """float64 decisions and which tokens they are decided for.  zc = lc + g2 carries lc's bound and the rounding of the noise add, za =
    la + g3 only the latter; a token counts where its top-1 / top-2 margin exceeds TWICE the largest error of its row (each of the two
    competing values may move by the bound)."""
    zc, za = lc + g2.double(), la_rows.double() + g3.double()
    bc = (lc_bound + U32 * zc.abs()).amax(1)
    ba = (U32 * za.abs()).amax(1)
    return first_argmax(zc), first_argmax(za), margin(zc) > 2 * bc, margin(za) > 2 * ba


def high_level_gate(hl_rows, g1):
    """(mc, ma) = softmax(hl + g1) over the two columns -> (ref [N][2], bound [N][2]).  z = hl + g1: U32 |z| each; z - max: one more
    rounding; so the exponent moves by d = U32 (|z0| + |z1| + |z0 - z1|); exp: 3 U32 (libm-class, < 2 ulp, and the rounding); numerator and
    denominator each carry d + 3 U32, then the sum, the reciprocal (2 ulp) and the product:  bound = p (2 d + 10 U32)."""
    z = hl_rows.double() + g1.double()
    p = torch.softmax(z, 1)
    d = U32 * (z.abs().sum(1) + (z[:, 0] - z[:, 1]).abs())
    return p, p * (2 * d + 10 * U32).unsqueeze(1)


def count_table(ic, ia, E, pairs, block=256):
    """tokens per `block`-token block and expert pair ic * E + ia (pairs) or expert group ic / E + ia -> int64 [ceil(N / block)][G]"""
    N, G = ic.numel(), E * E if pairs else 2 * E
    blk = torch.arange(N) // block
    nblk = (N + block - 1) // block
    ic, ia = ic.long(), ia.long()
    if pairs:
        return torch.bincount(blk * G + ic * E + ia, minlength=nblk * G).view(nblk, G)
    return (torch.bincount(blk * G + ic, minlength=nblk * G) + torch.bincount(blk * G + E + ia, minlength=nblk * G)).view(nblk, G)


MARGIN_CAP = 0.05      # share of tokens the margin rule may exclude


def caption_case(T, E, NS=640, K=768, Hh=8, Beff=2):
    """The caption-gate inputs of the GPU tests (one clip, two branches with different captions), shared with the host test that asserts
    the margin cap on the reference alone.  Scales: keys 0.01 keep a score's accumulation error (~ K U32 sum |x| |key|) near 5e-4, so
    the logit bound stays near 0.02 against logit differences of order 0.5 and Gumbel noise of spread 1.3."""
    N, B = Beff * T, 1
    tag = f"cg{T}_{E}"
    c = dict(T=T, E=E, NS=NS, K=K, Hh=Hh, Beff=Beff, B=B, N=N, la_rows=B * T, hl_ld=6)
    c["x"] = rnd((N, K), tag + "x").bfloat16()
    c["keys"] = rnd((Beff, NS, K), tag + "k", 0.01).bfloat16()
    c["sbias"] = rnd((Beff, NS), tag + "sb", 0.3).float()
    c["vw"] = rnd((Beff, NS, E), tag + "vw", 2.0).float()
    c["bg"] = rnd((E,), tag + "bg", 0.3).float()
    c["la"] = rnd((B * T, E), tag + "la").float()
    c["hl"] = rnd((Beff, c["hl_ld"]), tag + "hl").float()
    gum = lambda w, s: -torch.from_numpy(prng.exponential(prng.key_seed(s, tag), N * w).reshape(N, w)).log()
    c["g1"], c["g2"], c["g3"] = gum(2, 1).float(), gum(E, 2).float(), gum(E, 3).float()
    return c


def caption_reference(c):
    """everything the tests compare with, from a caption_case: computed once per case"""
    n = torch.arange(c["N"])
    lc, lcb = caption_logits(c["x"], c["keys"], c["sbias"], c["vw"], c["bg"], c["T"], c["Hh"])
    ic, ia, okc, oka = routing(lc, lcb, c["la"][n % c["la_rows"]], c["g2"], c["g3"])
    p, pb = high_level_gate(c["hl"][n // c["T"], :2], c["g1"])
    return dict(lc=lc, lc_bound=lcb, ic=ic, ia=ia, ok_c=okc, ok_a=oka, p=p, p_bound=pb)


def excluded_share(ref):
    return 1.0 - float(ref["ok_c"].double().mean()), 1.0 - float(ref["ok_a"].double().mean())


def worst(err, bound):
    """largest err / bound over the finite entries (0 / 0 counts as 0)"""
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = r[~torch.isnan(r)]
    return float(r.max()) if r.numel() else 0.0
