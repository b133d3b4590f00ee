"""The bounds of tests/moe_oracles.py, checked against the reference alone (no kernel, no GPU): a torch fp32 emulation of every stage -
bf16 operands, fp32 matmul, the same bf16 rounding points - lies inside the stage's bound at every element, and deliberately wrong
emulations (a 64-wide K slab dropped for the rows of the last tile, two token rows swapped, the gate row of the neighbouring clip at a
clip boundary) fall outside it on the affected rows.  So the bounds are neither vacuous nor too tight for a correct fp32 implementation."""
import pytest
import torch

from tests import moe_oracles as O


def silu32(a):
    return a * torch.sigmoid(a)


def outside(err, bound, rows):
    """every one of `rows` has elements outside the bound"""
    return bool((err[rows] > bound[rows]).any(1).all())


def inside_elsewhere(err, bound, rows):
    keep = torch.ones(err.shape[0], dtype=torch.bool)
    keep[rows] = False
    return bool((err[keep] <= bound[keep]).all())


# ------------------------------------------------------------------------------------------------------------------ band FFN
def band_case(M, H, E, band, T):
    D, ld = E * band, E * band + 8
    y = O.rnd((M, ld), "by").bfloat16()
    w13 = O.rnd((E, 2 * H, band), "bw13", band ** -0.5).bfloat16()
    w2 = O.rnd((E, band, H), "bw2", H ** -0.5).bfloat16()
    gate = O.rnd(((M + T - 1) // T + 1, ld), "bg").float()
    out_in = O.rnd((M, D), "bo").float()
    return y, w13, w2, gate, out_in


def band_emul(y, w13, w2, gate, out_in, T, E, band, drop=None, clip_shift=None):
    """fp32 emulation.  drop = (first row, k0): hidden columns [k0, k0 + 64) left out of the second product from that row on;
    clip_shift = (rows, d): those rows read the gate of clip m // T + d."""
    M = y.shape[0]
    clip = torch.arange(M) // T
    if clip_shift is not None:
        clip = clip.clone()
        clip[clip_shift[0]] += clip_shift[1]
    out = torch.empty(M, E * band)
    for e in range(E):
        cols = slice(e * band, (e + 1) * band)
        ye = y[:, cols].float()
        a, b = ye @ w13[e, 0::2].float().T, ye @ w13[e, 1::2].float().T
        h = (silu32(a) * b).bfloat16().float()
        if drop is not None:
            h[drop[0]:, drop[1]:drop[1] + 64] = 0
        z = h @ w2[e].float().T
        out[:, cols] = (out_in[:, cols].double() + gate[clip][:, cols].double() * z.double()).float()      # one rounding: the kernel's fma
    return out.double()


@pytest.mark.parametrize("M,H,E,band", [(193, 64, 4, 192), (257, 512, 8, 96), (130, 128, 1, 192)])
def test_band_ffn_bound_holds_for_fp32_and_rejects_wrong_results(M, H, E, band):
    T = 100
    case = band_case(M, H, E, band, T)
    ref, bound = O.band_ffn(*case, T, E, band)
    assert bool((bound > 0).all())
    err = (band_emul(*case, T, E, band) - ref).abs()
    print(f"band_ffn fp32 emulation M={M} H={H} E={E} band={band}: worst err / bound = {O.worst(err, bound):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements of a correct fp32 evaluation outside the bound"
    rows = 192 if band == 192 else 256                                  # token rows of a workgroup
    last = torch.arange((M - 1) // rows * rows, M)                      # the rows of the last tile
    err = (band_emul(*case, T, E, band, drop=(int(last[0]), H - 64)) - ref).abs()
    assert outside(err, bound, last) and inside_elsewhere(err, bound, last), "a dropped 64-wide K slab in the last tile went unnoticed"
    good = band_emul(*case, T, E, band)
    swapped = good.clone()
    swapped[[3, M - 2]] = good[[M - 2, 3]]
    err = (swapped - ref).abs()
    assert outside(err, bound, torch.tensor([3, M - 2])) and inside_elsewhere(err, bound, torch.tensor([3, M - 2])), "two swapped rows went unnoticed"
    for rows_, d in ((torch.tensor([T - 1]), 1), (torch.tensor([T]), -1)):       # the last token of clip 0, the first of clip 1
        err = (band_emul(*case, T, E, band, clip_shift=(rows_, d)) - ref).abs()
        assert outside(err, bound, rows_) and inside_elsewhere(err, bound, rows_), f"the gate of clip m // T {d:+d} at a clip boundary went unnoticed"


# ------------------------------------------------------------------------------------------------------------------ routed pair FFN
def pair_case(E, H, D, counts):
    """tokens of every (caption, acoustic) pair bucket scattered over the token order -> operands and the bucketing, built on the host the
    way the bucket kernel lays it out (caption slots = pair buckets caption-major, acoustic slots the same buckets acoustic-major)"""
    N = sum(counts)
    order = O.rnd((N,), "porder").argsort()
    pair = torch.empty(N, dtype=torch.long)
    pair[order] = torch.repeat_interleave(torch.arange(E * E), torch.tensor(counts))
    ic, ia = pair // E, pair % E
    slot_c = torch.cat([(pair == g).nonzero().squeeze(1) for g in range(E * E)])
    slot_a = torch.cat([(pair == c * E + a).nonzero().squeeze(1) for a in range(E) for c in range(E)])
    perm = torch.cat([slot_c, slot_a])
    where_a = torch.empty(N, dtype=torch.long)
    where_a[slot_a] = N + torch.arange(N)
    pair_pa = where_a[slot_c]
    pair_off = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(pair, minlength=E * E).cumsum(0)])
    group_off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cat([torch.bincount(ic, minlength=E), torch.bincount(ia, minlength=E)]).cumsum(0)])
    u = O.rnd((N, D), "pu").bfloat16()
    w13 = O.rnd((2 * E, 2 * H, D), "pw13", D ** -0.5).bfloat16()
    w2 = O.rnd((2 * E, D, H), "pw2", H ** -0.5).bfloat16()
    mc = torch.sigmoid(O.rnd((N,), "pmc")).float() * 0.9 + 0.05
    return dict(N=N, E=E, H=H, D=D, u=u, w13=w13, w2=w2, mc=mc, ma=(1 - mc).float(), perm=perm, pair_pa=pair_pa, pair_off=pair_off,
                group_off=group_off, ic=ic, ia=ia)


def swiglu_emul(c, drop=None):
    """drop = (first slot, k0): u columns [k0, k0 + 64) left out from that slot on"""
    N, H = c["N"], c["H"]
    out = torch.zeros(2 * N, H)
    for g in range(2 * c["E"]):
        slots = torch.arange(int(c["group_off"][g]), int(c["group_off"][g + 1]))
        if not slots.numel():
            continue
        tok = c["perm"][slots]
        x = c["u"][tok].float()
        if drop is not None:
            x[slots >= drop[0], drop[1]:drop[1] + 64] = 0
        a, b = x @ c["w13"][g, 0::2].float().T, x @ c["w13"][g, 1::2].float().T
        m = torch.where(slots < N, c["mc"][tok], c["ma"][tok]).unsqueeze(1)
        out[slots] = (silu32(a) * b * m).bfloat16().float()
    return out.double()


def w2_emul(c, hs, drop=None):
    """drop = (first pair slot, k0): hidden columns [k0, k0 + 64) of the caption half left out from that slot on"""
    N, E = c["N"], c["E"]
    out = torch.full((N, c["D"]), float("nan"))
    for g in range(E * E):
        p = torch.arange(int(c["pair_off"][g]), int(c["pair_off"][g + 1]))
        if not p.numel():
            continue
        A, Bm = hs[p].float(), hs[c["pair_pa"][p]].float()
        if drop is not None:
            A[p >= drop[0], drop[1]:drop[1] + 64] = 0
        x = torch.cat([A, Bm], 1) @ torch.cat([c["w2"][g // E], c["w2"][E + g % E]], 1).float().T       # one accumulator, K = 2H
        out[c["perm"][p]] = x.bfloat16().float()
    return out.double()


@pytest.mark.parametrize("E,H,D,counts", [(2, 64, 400, [0, 1, 129, 40]), (4, 128, 192, [0, 1, 127, 128, 129, 3, 0, 17, 5, 2, 0, 9, 1, 30, 20, 4])])
def test_routed_pair_bounds_hold_for_fp32_and_reject_wrong_results(E, H, D, counts):
    c = pair_case(E, H, D, counts)
    N = c["N"]
    # first stage: SwiGLU with the gate weight folded in
    ref, bound = O.swiglu_folded(c["u"], c["perm"], c["group_off"], c["w13"], c["mc"], c["ma"], N)
    hs = swiglu_emul(c)
    err = (hs - ref).abs()
    print(f"swiglu_folded fp32 emulation E={E} H={H} D={D}: worst err / bound = {O.worst(err, bound):.3f}, "
          f"{int((err > 0).sum())} of {err.numel()} hidden values on a neighbouring bf16")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} hidden values of a correct fp32 evaluation outside the bound"
    big = max(range(2 * E), key=lambda g: int(c["group_off"][g + 1] - c["group_off"][g]))
    lo, hi = int(c["group_off"][big]), int(c["group_off"][big + 1])
    last = torch.arange(lo + (hi - lo - 1) // 128 * 128, hi)            # the rows of the group's last 128-row tile
    err = (swiglu_emul(c, drop=(int(last[0]), D - 64)) - ref).abs()
    tail = torch.arange(int(last[0]), 2 * N)
    assert outside(err, bound, last) and inside_elsewhere(err, bound, tail), "a dropped 64-wide K slab went unnoticed"
    swapped = hs.clone()
    swapped[[lo, hi - 1]] = hs[[hi - 1, lo]]
    err = (swapped - ref).abs()
    assert outside(err, bound, torch.tensor([lo, hi - 1])) and inside_elsewhere(err, bound, torch.tensor([lo, hi - 1])), "two swapped rows went unnoticed"
    wrong = hs.clone()                                                  # the other gate weight: ma where mc belongs
    wrong[:N] = (hs[:N] / c["mc"][c["perm"][:N]].double().unsqueeze(1) * c["ma"][c["perm"][:N]].double().unsqueeze(1))
    off = ((c["mc"] - c["ma"]).abs() > 0.1)[c["perm"][:N]].nonzero().squeeze(1)
    assert outside((wrong - ref).abs(), bound, off), "the acoustic gate weight in a caption slot went unnoticed"
    # second stage, on the hidden values of the first
    hs16 = hs.bfloat16()
    ref2, bound2 = O.pair_w2(hs16, c["w2"], c["perm"], c["pair_off"], c["pair_pa"], N, E)
    assert not torch.isnan(ref2).any()
    out = w2_emul(c, hs16)
    err = (out - ref2).abs()
    print(f"pair_w2 fp32 emulation E={E} H={H} D={D}: worst err / bound = {O.worst(err, bound2):.3f}")
    assert bool((err <= bound2).all()), f"{int((err > bound2).sum())} outputs of a correct fp32 evaluation outside the bound"
    g = max(range(E * E), key=lambda g: counts[g])
    plo, phi = int(c["pair_off"][g]), int(c["pair_off"][g + 1])
    last = torch.arange(plo + (phi - plo - 1) // 128 * 128, phi)
    err = (w2_emul(c, hs16, drop=(int(last[0]), H - 64)) - ref2).abs()
    bad = c["perm"][torch.arange(int(last[0]), N)]
    assert outside(err, bound2, c["perm"][last]) and inside_elsewhere(err, bound2, bad), "a dropped 64-wide K slab in the last tile went unnoticed"
    t1, t2 = int(c["perm"][plo]), int(c["perm"][phi - 1])
    swapped = out.clone()
    swapped[[t1, t2]] = out[[t2, t1]]
    err = (swapped - ref2).abs()
    assert outside(err, bound2, torch.tensor([t1, t2])) and inside_elsewhere(err, bound2, torch.tensor([t1, t2])), "two swapped rows went unnoticed"


# ------------------------------------------------------------------------------------------------------------------ caption gate
def gate_emul(c, clip_shift=None, drop=None):
    """drop = (rows, k0): feature columns [k0, k0 + 64) of those token rows left out of the scores"""
    N, T, Hh, E = c["N"], c["T"], c["Hh"], c["E"]
    x = c["x"].float()
    if drop is not None:
        x[drop[0], drop[1]:drop[1] + 64] = 0
    clip = torch.arange(N) // T
    if clip_shift is not None:
        clip = clip.clone()
        clip[clip_shift[0]] += clip_shift[1]
    s = torch.empty(N, c["NS"])
    for b in range(c["Beff"]):
        s[clip == b] = x[clip == b] @ c["keys"][b].float().T + c["sbias"][b]
    q = torch.softmax(s.view(N, -1, Hh), 1)
    return (torch.einsum("nlh,nlhe->ne", q, c["vw"][clip].view(N, -1, Hh, E)) + c["bg"]).double()


@pytest.mark.parametrize("T,E", [(1, 4), (64, 4), (130, 4), (130, 8)])
def test_caption_gate_bound_margin_cap_and_wrong_clip(T, E):
    """the shapes of the GPU tests: the fp32 emulation's logits lie inside the bound, its decisions equal the float64 ones wherever the
    margin rule decides, the rule excludes at most 5 % of the tokens of the REFERENCE, and a token that reads the other branch's caption
    operands at the clip boundary falls outside the bound"""
    c = O.caption_case(T, E)
    ref = O.caption_reference(c)
    xc, xa = O.excluded_share(ref)
    print(f"caption gate T={T} E={E}: margin rule excludes {100 * xc:.2f} % (caption) / {100 * xa:.2f} % (acoustic) of {c['N']} tokens; "
          f"largest logit bound {float(ref['lc_bound'].max()):.3e}")
    assert xc <= O.MARGIN_CAP and xa <= O.MARGIN_CAP
    lc = gate_emul(c)
    err = (lc - ref["lc"]).abs()
    print(f"caption logits fp32 emulation: worst err / bound = {O.worst(err, ref['lc_bound']):.3g}")
    assert bool((err <= ref["lc_bound"]).all())
    n = torch.arange(c["N"])
    ic = O.first_argmax(lc.float() + c["g2"])
    ia = O.first_argmax(c["la"][n % c["la_rows"]] + c["g3"])
    assert torch.equal(ic[ref["ok_c"]], ref["ic"][ref["ok_c"]]) and torch.equal(ia[ref["ok_a"]], ref["ia"][ref["ok_a"]])
    p32 = torch.softmax(c["hl"][n // T, :2] + c["g1"], 1).double()
    assert bool(((p32 - ref["p"]).abs() <= ref["p_bound"]).all())
    assert bool(((ref["p"] > 0) & (ref["p"] < 1)).all())
    for rows, d in ((torch.tensor([T - 1]), 1), (torch.tensor([T]), -1)):
        err = (gate_emul(c, clip_shift=(rows, d)) - ref["lc"]).abs()
        assert outside(err, ref["lc_bound"], rows) and inside_elsewhere(err, ref["lc_bound"], rows), "the neighbouring clip's caption went unnoticed"
    last = torch.arange((c["N"] - 1) // 64 * 64 if T > 64 else c["N"] - 1, c["N"])      # the rows of the last 64-token tile
    err = (gate_emul(c, drop=(last, c["K"] - 64)) - ref["lc"]).abs()
    assert outside(err, ref["lc_bound"], last) and inside_elsewhere(err, ref["lc_bound"], last), "a dropped 64-wide K slab of the scores went unnoticed"


def test_count_table_and_first_maximum():
    ic, ia = torch.tensor([0, 1, 1, 3] * 65), torch.tensor([2, 2, 0, 1] * 65)
    t = O.count_table(ic, ia, 4, True)
    assert t.shape == (2, 16) and int(t.sum()) == 260 and int(t[1].sum()) == 4 and int(t[0, 0 * 4 + 2]) == 64
    t = O.count_table(ic, ia, 4, False)
    assert t.shape == (2, 8) and int(t.sum()) == 520 and int(t[0, 1]) == 128 and int(t[0, 4 + 2]) == 128
    assert O.first_argmax(torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]])).tolist() == [1, 0]
    assert O.margin(torch.tensor([[1.0, 3.0, 3.5, 2.0]])).tolist() == [0.5]
