"""The bounds of tests/attn_oracles.py, checked against the reference alone (no kernel, no GPU), on the input sets of
tests/test_gpu_attention_units.py: a torch fp32 emulation of attn_kernel's arithmetic - 64-key tiles, base-2 online softmax with the
deferred rescale decided per 32-row wave at threshold 0 and 8, p rounded to bf16 (or split hi + lo) for the product only, fp32 row sum,
the cross result normalised and weighted before the self pass, one final rounding - and of the QKV + RoPE epilogue lies inside the bound
at every element, and every listed wrong result (computed in float64 from deliberately wrong operands, rounded to planes like a device
result) leaves the bound by at least 2x on at least one element of every (row, head) designated for it.  Nothing is excluded from any check
(the margin rule's excluded share is zero).  Each case prints its worst err / bound and its smallest mutation factor (pytest -s)."""
import math

import pytest
import torch

from tests import attn_oracles as A
from versband_amd import pack

FACTOR = 2.0          # a wrong result must exceed the bound by this on its designated rows


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def emul_pass(qp, kp, vp, nk, thr):
    """one (batch row)'s pass over its first nk keys: qp [np][H][R][hd], kp / vp [np][H][S][hd] fp32 planes -> (acc [H][R][hd], l [H][R])"""
    np_, H, R, hd = qp.shape
    c32 = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt()) * torch.tensor(A.LOG2E, dtype=torch.float32)
    nt = (nk + A.KT - 1) // A.KT
    pad = lambda x, fill: torch.cat([x[:, :, :nk], torch.full((np_, H, nt * A.KT - nk, hd), fill)], 2)
    kp, vp = pad(kp, 0.0), pad(vp, 0.0)
    vp[0, :, nk:] = A.BIG                                                  # the pad columns of V^T: finite, never zero
    m = torch.full((H, R), -1e30)
    l, o = torch.zeros(H, R), torch.zeros(H, R, hd)
    for kt in range(nt):
        ks = slice(kt * A.KT, (kt + 1) * A.KT)
        s = qp[0] @ kp[0][:, ks].transpose(1, 2)
        if np_ == 2:
            s = s + qp[0] @ kp[1][:, ks].transpose(1, 2) + qp[1] @ kp[0][:, ks].transpose(1, 2)
        s[:, :, max(nk - kt * A.KT, 0):] = -float("inf")
        m_new = torch.maximum(m, s.amax(-1) * c32)
        need = ~(m_new <= m + thr)                                         # per row; the kernel decides per wave of 32 query rows
        wave = torch.arange(R) // 32
        for w in range(int(wave.max()) + 1):
            need[:, wave == w] = need[:, wave == w].any(1, keepdim=True)
        alpha = torch.where(need, torch.exp2(m - m_new), torch.ones_like(m))
        m = torch.where(need, m_new, m)
        e = torch.exp2((s.double() * c32.double() - m.double().unsqueeze(-1)).float())        # the fma: one rounding
        l = l * alpha + e.sum(-1)
        ph = e.bfloat16().float()
        pv = ph @ vp[0][:, ks]
        if np_ == 2:
            pv = pv + ph @ vp[1][:, ks] + (e - ph).bfloat16().float() @ vp[0][:, ks]
        o = o * alpha.unsqueeze(-1) + pv
    return o, l


def emul_attention(c, np_, thr, use_self, use_cross):
    """-> [B][T][H][hd] float64: the value of the output planes; rows >= lens[b] NaN"""
    B, T, H = c["B"], c["T"], c["H"]
    pl = {n: pack.to_planes(c[n], np_).float().permute(0, 1, 3, 2, 4) for n in ("q", "k", "v", "ky", "vy")}     # [np][B][H][.][hd]
    out = torch.full((B, H, T, A.HD), float("nan"), dtype=torch.float64)
    for b in range(B):
        n = T if c["lens"] is None else c["lens"][b]
        q = pl["q"][:, b, :, :n]
        o = torch.zeros(H, n, A.HD)
        if use_cross:
            oc, lc = emul_pass(q, pl["ky"][:, b], pl["vy"][:, b], c["Lc"], thr)
            o = oc * (c["cw"].view(H, 1) / lc).unsqueeze(-1)
        if use_self:
            os_, ls = emul_pass(q, pl["k"][:, b], pl["v"][:, b], n, thr)
            o = os_ * (1.0 / ls).unsqueeze(-1) + o
        out[b, :, :n] = A.planes_r(o.double(), np_)
    return out.permute(0, 2, 1, 3)


def inside(what, got, ref, bound):
    ok = ~torch.isnan(ref)
    assert bool((torch.isnan(got) == torch.isnan(ref)).all()), f"{what}: defined rows differ"
    err = (got - ref).abs()[ok]
    ratio = A.worst(err, bound[ok])
    print(f"{what}: worst err / bound = {ratio:.3f}")
    assert bool((err <= bound[ok]).all()), f"{what}: {int((err > bound[ok]).sum())} of {err.numel()} elements of a correct fp32 evaluation outside the bound"
    return ratio


ALL_ATTN = [(c, None) for c in A.PLAIN_CASES] + [((len(A.LENS), A.LENS_H, A.LENS_T, A.LENS_LC), A.LENS)]


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("case,lens", ALL_ATTN)
def test_attention_bound_holds_for_the_fp32_emulation(case, lens, np_):
    c = A.attn_case(*case, lens)
    for use_self, use_cross in (A.MODES if lens is None else [(True, True)]):
        ref, bound = A.attn_reference(*case, lens, np_, use_self, use_cross)
        assert bool((bound[~torch.isnan(bound)] > 0).all())
        for thr in (0.0, A.THR):
            inside(f"attention {case} lens={lens is not None} np={np_} self={use_self} cross={use_cross} thr={thr:g}",
                   emul_attention(c, np_, thr, use_self, use_cross), ref, bound)


# ------------------------------------------------------------------------------------------------------------------ planted keys
def planted_mask(c, cross, keys=None):
    """[B][T][H] mask of the query rows planted for the boundary keys (all of them, or those in `keys`) of the self / cross pass"""
    m = torch.zeros(c["B"], c["T"], c["H"], dtype=torch.bool)
    for b in range(c["B"]):
        n = c["T"] if c["lens"] is None else c["lens"][b]
        for j, r in A.planted_rows(n, c["Lc"] if cross else n, cross).items():
            if keys is None or j in keys(c["Lc"] if cross else n):
                m[b, r] = True
    return m


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("case,lens", ALL_ATTN)
def test_planted_boundary_keys_carry_a_quarter_of_their_row(case, lens, np_):
    c = A.attn_case(*case, lens)
    pv = {n: A.plane_values(c[n], np_).permute(0, 2, 1, 3) for n in ("q", "k", "v", "ky", "vy")}
    for b in range(c["B"]):
        n = c["T"] if lens is None else lens[b]
        for cross, (kk, vv, S) in ((False, (pv["k"][b, :, :n], pv["v"][b, :, :n], n)), (True, (pv["ky"][b], pv["vy"][b], c["Lc"]))):
            P = A.softmax_pass(pv["q"][b, :, :n], kk, vv, np_)[2]            # [H][n][S]
            for j, r in A.planted_rows(n, S, cross).items():
                assert float(P[:, r, j].min()) >= 0.25, f"batch row {b} {'cross' if cross else 'self'} key {j} row {r}: share {float(P[:, r, j].min()):.3f}"


# ------------------------------------------------------------------------------------------------------------------ wrong results
def factor(what, wrong, ref, bound, mask):
    """smallest over the designated (b, t, h) of the largest err / bound over d; asserted >= FACTOR"""
    assert bool(mask.any()), f"{what}: no designated row"
    r = ((wrong - ref).abs() / bound)
    r = torch.where(torch.isnan(wrong) & ~torch.isnan(ref), torch.full_like(r, float("inf")), r).amax(-1)[mask]
    assert not bool(torch.isnan(r).any()), f"{what}: a designated row is undefined in the reference"
    f = float(r.min())
    assert f >= FACTOR, f"{what}: exceeds the bound by {f:.2f}x only on a designated row (need {FACTOR:g}x)"
    return f


def drop_key(x, j):
    return torch.cat([x[:, :j], x[:, j + 1:]], 1)


def wrong_results(c, np_):
    """-> [(name, wrong [B][T][H][hd], designated mask [B][T][H])] for self + cross on the case's plane values"""
    B, T, H, Lc, lens = c["B"], c["T"], c["H"], c["Lc"], c["lens"]
    q, k, v, ky, vy = (A.plane_values(c[n], np_) for n in ("q", "k", "v", "ky", "vy"))
    cw = c["cw"]
    att = lambda **kw: A.planes_r(A.attention(kw.get("q", q), kw.get("k", k), kw.get("v", v), kw.get("ky", ky), kw.get("vy", vy), kw.get("cw", cw),
                                              lens, np_, kw.get("key_lens"))[0], np_)
    ns = [T if lens is None else n for n in (lens or [T] * B)]
    every = torch.zeros(B, T, H, dtype=torch.bool)
    for b, n in enumerate(ns):
        every[b, :n] = True
    last = lambda n: (n - 1,)
    quiet = torch.zeros(B, T, H, dtype=torch.bool)                           # where a pad key of score 0 must show
    for b, n in enumerate(ns):
        if A.quiet_row(n, Lc) is not None:
            quiet[b, A.quiet_row(n, Lc)] = True
    out = []
    if min(ns) >= 2 or lens is not None:
        m = planted_mask(c, False, last) & torch.tensor([n >= 2 for n in ns]).view(B, 1, 1)
        out.append(("last valid self key dropped", att(key_lens=[max(n - 1, 1) for n in ns]), m))
        if lens is not None:
            out.append(("row length one short", att(key_lens=[max(n - 1, 1) for n in ns]), m))
    if Lc >= 2:
        out.append(("last valid cross key dropped", att(ky=ky[:, :Lc - 1], vy=vy[:, :Lc - 1]), planted_mask(c, True, last)))
    pad_row = lambda x, fill: torch.cat([x, torch.full((B, 1, H, A.HD), fill, dtype=torch.float64)], 1)
    if lens is None:
        out.append(("first self pad key admitted with score 0", att(k=pad_row(k, 0.0), v=pad_row(v, A.BIG)), quiet))
    else:      # a length one too long reads the key behind the row's end; a key whose score is far below the row's maximum weighs nothing
        sc = torch.stack([torch.einsum("thd,hd->th", q[b], k[b, min(n, T - 1)]) for b, n in enumerate(ns)]) > 0
        m = every & sc & torch.tensor([n < T for n in ns]).view(B, 1, 1)
        assert float(m.double().sum()) >= 0.25 * float((every & torch.tensor([n < T for n in ns]).view(B, 1, 1)).double().sum())
        out.append(("row length one long", att(key_lens=[min(n + 1, T) for n in ns]), m))
    out.append(("first cross pad key admitted with score 0", att(ky=pad_row(ky, 0.0), vy=pad_row(vy, A.BIG)), quiet))
    for j in (A.KT - 1, A.KT):
        if lens is None and T > j + 1:
            out.append((f"self key {j} dropped", att(k=drop_key(k, j), v=drop_key(v, j)), planted_mask(c, False, lambda n: (j,))))
        if Lc > j + 1:
            out.append((f"cross key {j} dropped", att(ky=drop_key(ky, j), vy=drop_key(vy, j)), planted_mask(c, True, lambda n: (j,))))
    good = att()
    if min(ns) >= 2:
        sw, m = good.clone(), torch.zeros(B, T, H, dtype=torch.bool)
        for b, n in enumerate(ns):
            sw[b, [0, n - 1]] = good[b, [n - 1, 0]]
            m[b, [0, n - 1]] = True
        out.append(("two query rows swapped", sw, m))
    both = planted_mask(c, False) | planted_mask(c, True)
    if H >= 2:
        out.append(("the neighbouring head's V", att(v=v.roll(1, 2), vy=vy.roll(1, 2)), both))
        out.append(("the neighbouring head's cross_w", att(cw=cw.roll(1)), planted_mask(c, True)))
    if B >= 2:
        out.append(("the neighbouring batch row's cross keys", att(ky=ky.roll(1, 0)), planted_mask(c, True)))
    joint = torch.full((B, T, H, A.HD), float("nan"), dtype=torch.float64)
    for b, n in enumerate(ns):
        kk, vv = torch.cat([k[b, :n], ky[b]]).permute(1, 0, 2), torch.cat([v[b, :n], vy[b] * cw.double().view(1, H, 1)]).permute(1, 0, 2)
        joint[b, :n] = (torch.softmax(q[b, :n].permute(1, 0, 2) @ kk.transpose(1, 2) / math.sqrt(A.HD), -1) @ vv).permute(1, 0, 2)
    out.append(("one joint softmax over self and cross keys", A.planes_r(joint, np_), both))
    return out


MUT_CASES = [(c, None) for c in A.PLAIN_CASES if c[2] > 1] + [ALL_ATTN[-1]]


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("case,lens", MUT_CASES)
def test_attention_bound_rejects_wrong_results(case, lens, np_):
    c = A.attn_case(*case, lens)
    ref, bound = A.attn_reference(*case, lens, np_, True, True)
    worst = float("inf")
    for name, wrong, mask in wrong_results(c, np_):
        f = factor(f"{case} np={np_}: {name}", wrong, ref, bound, mask)
        print(f"attention {case} lens={lens is not None} np={np_}: {name}: {f:.3g}x the bound on {int(mask.sum())} designated (row, head)s")
        worst = min(worst, f)
    print(f"attention {case} lens={lens is not None} np={np_}: smallest mutation factor {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------ QKV + RoPE
def emul_qkv(c, np_):
    B, T, H = c["B"], c["T"], c["H"]
    D = H * A.HD
    up, wp = pack.to_planes(c["u"], np_).float(), pack.to_planes(c["w"], np_).float()
    y = up[0] @ wp[0].T
    if np_ == 2:
        y = y + up[1] @ wp[0].T + up[0] @ wp[1].T
    t = torch.arange(B * T) % T
    cs, sn = c["cos"][t].repeat(1, H), c["sin"][t].repeat(1, H)
    res = []
    for sec in range(2):
        v0, v1 = y[:, sec * D:(sec + 1) * D:2], y[:, sec * D + 1:(sec + 1) * D:2]
        o0 = (v0.double() * cs.double() - (v1 * sn).double()).float()      # fmaf(v0, c, -(v1 * s)): the product rounded, then one fma
        o1 = (v0.double() * sn.double() + (v1 * cs).double()).float()
        res.append(A.planes_r(torch.stack([o0, o1], 2).reshape(B * T, D).double(), np_))
    vt = A.planes_r(y[:, 2 * D:].double(), np_).view(B, T, H, A.HD).permute(0, 2, 3, 1)
    return res[0], res[1], vt


ALL_QKV = [(B, T) for B, T, _ in A.QKV_CASES]


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("B,T", ALL_QKV + [(None, A.QKV_P8_T)])
def test_qkv_rope_bound_holds_for_the_fp32_emulation(B, T, np_):
    B = B or A.p8_min_clips()
    ref = A.qkv_reference(B, T, np_)
    for name, got, r, bd in zip(("q", "k", "vt"), emul_qkv(A.qkv_case(B, T), np_), ref[:3], ref[3:]):
        assert bool((bd > 0).all())
        inside(f"qkv_rope B={B} T={T} np={np_} {name}", got, r, bd)


def test_the_p8_case_is_the_smallest_batch_that_reaches_the_8_wave_kernel():
    B = A.p8_min_clips()
    assert B == 62 and (B * A.QKV_P8_T + 255) // 256 * 3 >= 96 > ((B - 1) * A.QKV_P8_T + 255) // 256 * 3


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("B,T,Tpad", A.QKV_CASES)
def test_qkv_rope_bound_rejects_wrong_results(B, T, Tpad, np_):
    c = A.qkv_case(B, T)
    H, hd = c["H"], A.HD
    D = H * hd
    u, w = A.plane_values(c["u"], np_), A.plane_values(c["w"], np_)
    q, k, vt, bq, bk, bvt = A.qkv_reference(B, T, np_)
    run = lambda cos, sin, ww=w, uu=u, bb=B: A.qkv_rope(uu, ww, cos, sin, bb, T, H, hd, np_)[:3]
    rows = lambda x: x.reshape(-1, x.shape[-1])                               # q / k: token rows; vt: (b, h, d) rows
    worst = float("inf")

    def check(name, wrong, parts=(0, 1, 2), sel=None):
        nonlocal worst
        for i in parts:
            r = ((rows(wrong[i]) - rows((q, k, vt)[i])).abs() / rows((bq, bk, bvt)[i])).amax(1)
            r = r if sel is None or i == 2 else r[sel]
            f = float(r.min())
            assert f >= FACTOR, f"qkv_rope B={B} T={T} np={np_}: {name}: {('q', 'k', 'vt')[i]} exceeds the bound by {f:.2f}x only on a designated row"
            worst = min(worst, f)
        print(f"qkv_rope B={B} T={T} np={np_}: {name}: ok")

    cos, sin = c["cos"][:T], c["sin"][:T]
    if B >= 2:      # m = b * T decomposed into (b - 1, T): table row T for q / k, and V^T column 0 of clip b never written
        cos_w, sin_w = cos.clone(), sin.clone()
        cos_w[0], sin_w[0] = c["cos"][T], c["sin"][T]
        wq, wk, _ = run(cos_w, sin_w)
        first = torch.arange(1, B) * T
        check("t of the wrong clip at m = b T", (wq, wk, None), (0, 1), first)
        wvt = vt.clone()
        wvt[1:, :, :, 0] = 0.0
        f = float(((wvt - vt).abs() / bvt)[1:, :, :, 0].amax((1, 2)).min())     # one element per (h, d) row: the column of clip b as a whole
        assert f >= FACTOR, f"an unwritten V^T column 0: {f:.2f}x"
        worst = min(worst, f)
    for d in (1, -1):
        check(f"pair rotated with j {d:+d}", run(cos.roll(d, 1), sin.roll(d, 1)), (0, 1))
    check("sin's sign flipped", run(cos, -sin), (0, 1))
    for d in (1, -1):
        check(f"head h {d:+d}", run(cos, sin, w.view(3, H, hd, D).roll(d, 1).reshape(3 * D, D)))
    if Tpad != T:
        buf = torch.zeros(B * H * hd * Tpad, dtype=torch.float64)
        buf[:vt.numel()] = vt.reshape(-1)                                    # rows written T apart into the buffer of pitch Tpad
        wrong = buf.view(B, H, hd, Tpad)[..., :T]
        r = ((rows(wrong) - rows(vt)).abs() / rows(bvt)).amax(1)[1:]         # (row 0 starts at the buffer's start either way)
        f = float(r.min())
        assert f >= FACTOR, f"V^T at pitch T instead of Tpad: {f:.2f}x"
        worst = min(worst, f)
    print(f"qkv_rope B={B} T={T} np={np_}: smallest mutation factor {worst:.3g}")
