"""The MoE block's fused kernels, each alone behind its C-ABI unit wrapper (vb_band_ffn, vb_routed_ffn_pair, vb_caption_gate), against the
stage-wise float64 oracles of tests/moe_oracles.py and their derived per-element bounds - at the small and ragged shapes the engine never
reaches (its eligibility rules take the fused kernels from ~6000 token rows on): one row, one row short of / past a tile, empty and
one-row pair buckets, one hidden chunk, clip boundaries inside a tile, leftover columns.  Every float input is followed by NaN guard
elements in its allocation, every output by sentinel rows / columns that must come back untouched.  Each case prints its worst
err / bound ratio (pytest -s)."""
import functools

import pytest
import torch

from tests import moe_oracles as O
from versband_amd import _lib as L

pytestmark = pytest.mark.gpu
GUARD = 4096          # guard elements behind every buffer
SENT = 12345.0        # sentinel of the fp32 guard rows / columns (NaN for bf16 outputs, -7 for indices)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


def guarded(t, fill=float("nan"), guard=GUARD):
    """device copy of t followed by `guard` elements of `fill` in the same allocation -> (the data as a view at its start, the whole buffer)"""
    flat = torch.full((t.numel() + guard,), fill, dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1)
    buf = flat.cuda()
    return buf[:t.numel()].view(t.shape), buf


def untouched(buf, n, fill):
    tail = buf[n:].cpu()
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def within(what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = O.worst(err, bound)
    print(f"{what}: worst err / bound = {ratio:.3g}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound (worst ratio {ratio:.3f})"
    return ratio


def tuned(knob, value, fn):
    """fn() under VB_<knob> = value (None: unset); the knob is removed again whatever happens"""
    try:
        L.set_tuning(**{knob: value})
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        L.set_tuning(**{knob: None})


# ------------------------------------------------------------------------------------------------------------------ band FFN
@functools.lru_cache(maxsize=None)
def band_case(M, H, E, band, T):
    D = E * band
    ldy, gate_ld, ldc = D + 8, D + 12, D + 4                            # every leading dimension wider than the D columns used
    y = O.rnd((M, ldy), "by").bfloat16()
    w13 = O.rnd((E, 2 * H, band), "bw13", band ** -0.5).bfloat16()
    w2 = O.rnd((E, band, H), "bw2", H ** -0.5).bfloat16()
    gate = O.rnd(((M + T - 1) // T, gate_ld), "bgate").float()
    out_in = O.rnd((M, ldc), "bout").float()                            # out32 starts non-zero
    ref, bound = O.band_ffn(y, w13, w2, gate, out_in, T, E, band)
    return dict(y=y, w13=w13, w2=w2, gate=gate, out_in=out_in, ref=ref, bound=bound, ldy=ldy, gate_ld=gate_ld, ldc=ldc)


def run_band(lib, c, M, H, E, band, T):
    ins = [guarded(c[k]) for k in ("y", "w13", "w2", "gate")]
    out, obuf = guarded(c["out_in"], SENT, 8 * c["ldc"])                # eight sentinel rows behind the M rows
    L.check(lib.vb_band_ffn(L.ptr(ins[0][0]), c["ldy"], L.ptr(ins[1][0]), L.ptr(ins[2][0]), M, H, E, band, L.ptr(ins[3][0]), c["gate_ld"], T,
                            L.ptr(out), c["ldc"], L.stream_ptr()), "band_ffn")
    torch.cuda.synchronize()
    assert untouched(obuf, out.numel(), SENT), "band_ffn wrote past row M"
    return out.cpu()


BAND_CASES = ([(192, 4, M, H) for M in (1, 191, 193, 385) for H in (64, 512)] + [(96, 8, M, H) for M in (1, 255, 257, 513) for H in (64, 512)] +
              [(192, 2, 385, 128), (192, 1, 385, 128)])       # E = 2 / 1: 4 / 8 row tiles share a group of 8 blocks (the engine never runs them)


@pytest.mark.parametrize("band,E,M,H", BAND_CASES)
def test_band_ffn_matches_float64(lib, band, E, M, H):
    """T = 100: clip boundaries fall inside the 192- / 256-row tiles and m // T runs through the reciprocal at a non-power of two; H = 64
    is one hidden chunk (the weight ring never wraps), 512 the model's.  band = 192: the hoisted and the two-pass epilogue give the same bits."""
    T, D = 100, E * band
    c = band_case(M, H, E, band, T)
    out = run_band(lib, c, M, H, E, band, T)
    assert bool(torch.isfinite(out).all()), "band_ffn read a guard value (or a row past M)"
    assert torch.equal(out[:, D:], c["out_in"][:, D:]), "band_ffn wrote past column E * band"
    within(f"band_ffn band={band} E={E} M={M} H={H}", out[:, :D], c["ref"], c["bound"])
    if band == 192:
        old = tuned("VB_BAND_EPI_OLD", "1", lambda: run_band(lib, c, M, H, E, band, T))
        assert torch.equal(old, out), "VB_BAND_EPI_OLD changes the bits"


# ------------------------------------------------------------------------------------------------------------------ routed pair FFN
PAIR_COUNTS = {4: (0, 1, 127, 128, 129, 3, 0, 17, 64, 65, 2, 0, 5, 1, 30, 20), 2: (0, 1, 129, 70), 1: (130,)}      # tokens per (c, a) bucket


@functools.lru_cache(maxsize=None)
def pair_case(E, H, D):
    counts = PAIR_COUNTS[E]
    N = sum(counts)
    order = O.rnd((N,), "porder").argsort()                             # the buckets' tokens, scattered over the token order
    pair = torch.empty(N, dtype=torch.long)
    pair[order] = torch.repeat_interleave(torch.arange(E * E), torch.tensor(counts))
    u = O.rnd((N, D), "pu").bfloat16()
    w13 = O.rnd((2 * E, 2 * H, D), "pw13", D ** -0.5).bfloat16()
    w2 = O.rnd((2 * E, D, H), "pw2", H ** -0.5).bfloat16()
    mc = (torch.sigmoid(O.rnd((N,), "pmc")) * 0.9 + 0.05).float()       # gate weights in (0.05, 0.95): positive, never 1
    return dict(N=N, ic=(pair // E).int(), ia=(pair % E).int(), u=u, w13=w13, w2=w2, mc=mc, ma=(1 - mc).float(), counts=counts)


def run_pair(lib, c, E, H, D):
    N = c["N"]
    ic, ia = c["ic"].cuda(), c["ia"].cuda()
    goff = torch.full((2 * E + 1,), -1, dtype=torch.int32, device="cuda")
    poff = torch.full((E * E + 1,), -1, dtype=torch.int32, device="cuda")
    perm = torch.full((2 * N + lib.vb_route_bucket_scratch_ints(N, E),), -1, dtype=torch.int32, device="cuda")
    ppa = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    L.check(lib.vb_route_bucket_pairs(L.ptr(ic), L.ptr(ia), N, E, L.ptr(goff), L.ptr(perm), L.ptr(poff), L.ptr(ppa), L.stream_ptr()), "bucket")
    torch.cuda.synchronize()
    assert poff.tolist() == [0] + torch.tensor(c["counts"]).cumsum(0).tolist()        # the bucket sizes the case is about
    ins = [guarded(c[k]) for k in ("u", "w13", "w2", "mc", "ma")]
    hid, hbuf = guarded(torch.full((2 * N, H), float("nan"), dtype=torch.bfloat16))
    out, obuf = guarded(torch.full((N, D), float("nan"), dtype=torch.bfloat16))
    L.check(lib.vb_routed_ffn_pair(L.ptr(ins[0][0]), L.ptr(perm), L.ptr(goff), L.ptr(poff), L.ptr(ppa), L.ptr(ins[1][0]), L.ptr(ins[2][0]),
                                   L.ptr(ins[3][0]), L.ptr(ins[4][0]), N, D, H, E, L.ptr(hid), L.ptr(out), L.stream_ptr()), "routed_ffn_pair")
    torch.cuda.synchronize()
    assert untouched(hbuf, hid.numel(), float("nan")) and untouched(obuf, out.numel(), float("nan")), "routed_ffn_pair wrote past its last row"
    return hid.cpu(), out.cpu(), perm.cpu()[:2 * N], goff.cpu(), poff.cpu(), ppa.cpu()


@pytest.mark.parametrize("E,H,D", [(4, 64, 768), (4, 512, 768), (4, 64, 400), (4, 512, 400), (2, 512, 768), (1, 64, 400)])
def test_routed_ffn_pair_matches_float64(lib, E, H, D):
    """E = 4: pair buckets of 0, 1, 127, 128 and 129 tokens among the sixteen.  D = 400 leaves 16 columns past the last whole 128-wide tile
    (and 16 past the second 192-wide one: VB_W2_PAIR=3 must not drop them).  The hidden rows are compared with the SwiGLU oracle, the
    output with the second product's oracle on the hidden rows the device wrote; VB_W2_PAIR = 2 (128-wide tiles) and 3 (192-wide) give
    the default's bits."""
    c = pair_case(E, H, D)
    N = c["N"]
    hid, out, perm, goff, poff, ppa = run_pair(lib, c, E, H, D)
    assert bool(torch.isfinite(hid.float()).all()) and bool(torch.isfinite(out.float()).all()), "an unwritten or guard-fed element"
    ref, bound = O.swiglu_folded(c["u"], perm, goff, c["w13"], c["mc"], c["ma"], N)
    within(f"swiglu_folded E={E} H={H} D={D}", hid, ref, bound)
    ref2, bound2 = O.pair_w2(hid, c["w2"], perm, poff, ppa, N, E)
    within(f"pair_w2 E={E} H={H} D={D}", out, ref2, bound2)
    for mode in ("2", "3"):
        hid_m, out_m = tuned("VB_W2_PAIR", mode, lambda: run_pair(lib, c, E, H, D))[:2]
        assert torch.equal(hid_m.view(torch.int16), hid.view(torch.int16)), f"hidden rows: VB_W2_PAIR={mode} vs the default"
        bad = (out_m.view(torch.int16) != out.view(torch.int16)).nonzero()
        assert not bad.numel(), f"VB_W2_PAIR={mode} vs the default: {bad.shape[0]} elements differ, first at {bad[0].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ caption gate
@functools.lru_cache(maxsize=None)
def gate_case(T, E):
    c = O.caption_case(T, E)
    return c, O.caption_reference(c)


def run_gate(lib, c, form, injected, pairs, want_lc=True):
    N, E, NS, K = c["N"], c["E"], c["NS"], c["K"]
    names = ("x", "keys", "sbias", "vw", "bg", "la", "hl") + (("g1", "g2", "g3") if injected else ())
    d = {k: guarded(c[k])[0] for k in names}
    g = [L.ptr(d[k]) if injected else None for k in ("g1", "g2", "g3")]
    G = E * E if pairs else 2 * E
    nblk = (N + 255) // 256
    ic, icb = guarded(torch.full((N,), -7, dtype=torch.int32), -7)
    ia, iab = guarded(torch.full((N,), -7, dtype=torch.int32), -7)
    mc, mcb = guarded(torch.full((N,), float("nan")))
    ma, mab = guarded(torch.full((N,), float("nan")))
    lc, lcb = guarded(torch.full((N, E), float("nan")))
    cnt, cntb = guarded(torch.zeros(nblk * G, dtype=torch.int32), 0)
    sc, scb = guarded(torch.full((N, NS), float("nan")))
    coff = torch.full((c["Beff"] + 1,), -1, dtype=torch.int32, device="cuda")
    lc_arg = L.ptr(lc) if form == 0 and want_lc else None
    L.check(lib.vb_caption_gate(L.ptr(d["x"]), L.ptr(d["keys"]), L.ptr(d["sbias"]), L.ptr(d["vw"]), L.ptr(d["bg"]), L.ptr(d["la"]), c["la_rows"],
                                L.ptr(d["hl"]), c["hl_ld"], g[0], g[1], g[2], 21, 3, 2, 1, c["Beff"], c["B"], c["T"], K, NS, c["Hh"], E, form,
                                L.ptr(sc), L.ptr(coff), L.ptr(ic), L.ptr(ia), L.ptr(mc), L.ptr(ma), lc_arg, L.ptr(cnt), G, int(pairs),
                                L.stream_ptr()), f"caption_gate form {form}")
    torch.cuda.synchronize()
    for what, buf, n, fill in (("ic", icb, N, -7), ("ia", iab, N, -7), ("mc", mcb, N, float("nan")), ("ma", mab, N, float("nan")),
                               ("lc_out", lcb, N * E, float("nan")), ("cnt", cntb, nblk * G, 0), ("scores", scb, N * NS, float("nan"))):
        assert untouched(buf, n, fill), f"caption_gate form {form} wrote past the end of {what}"
    return dict(ic=ic.cpu(), ia=ia.cpu(), mc=mc.cpu(), ma=ma.cpu(), lc=lc.cpu(), cnt=cnt.cpu().view(nblk, G))


def same_decisions(what, a, b):
    for k in ("ic", "ia", "cnt"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs at {int((a[k] != b[k]).sum())} places"
    for k in ("mc", "ma"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs in its bits"


def check_gate(what, c, ref, r, pairs, lc32):
    """decisions of one run against the device's own fp32 logits (every token), the float64 reference (every token the margin rule
    decides) and the derived bounds; lc32: the fp32 logits form 0 wrote"""
    N, E, T = c["N"], c["E"], c["T"]
    n = torch.arange(N)
    assert int(r["ic"].min()) >= 0 and int(r["ic"].max()) < E and int(r["ia"].min()) >= 0 and int(r["ia"].max()) < E
    assert bool(torch.isfinite(r["mc"]).all()) and bool(torch.isfinite(r["ma"]).all())
    assert torch.equal(r["ic"].long(), O.first_argmax(lc32 + c["g2"])), f"{what}: ic is not the first maximum of the device's own logits + noise"
    assert torch.equal(r["ia"].long(), O.first_argmax(c["la"][n % c["la_rows"]] + c["g3"])), f"{what}: ia is not the first maximum of la + noise"
    okc, oka = ref["ok_c"], ref["ok_a"]
    assert torch.equal(r["ic"].long()[okc], ref["ic"][okc]), f"{what}: ic differs from float64 on {int((r['ic'].long()[okc] != ref['ic'][okc]).sum())} decided tokens"
    assert torch.equal(r["ia"].long()[oka], ref["ia"][oka]), f"{what}: ia differs from float64 on decided tokens"
    within(f"{what} mc/ma", torch.stack([r["mc"], r["ma"]], 1), ref["p"], ref["p_bound"])
    assert torch.equal(r["cnt"].long(), O.count_table(r["ic"], r["ia"], E, pairs)), f"{what}: count table"


@pytest.mark.parametrize("T", [1, 64, 130])
def test_caption_gate_matches_float64_in_both_forms(lib, T):
    """NS = 640, K = 768, 8 heads, E = 4, one clip x two branches with different captions.  T = 1: one-token tiles; 64: exactly one tile of
    the one-launch kernel per branch; 130: 260 tokens = two 256-token count blocks, the second with four tokens, and a ragged tile at the
    clip boundary.  Injected noise: form 0's logits against float64, both forms' decisions; device-drawn noise: the forms agree bit for bit."""
    c, ref = gate_case(T, 4)
    xc, xa = O.excluded_share(ref)
    assert xc <= O.MARGIN_CAP and xa <= O.MARGIN_CAP
    print(f"caption gate T={T}: the margin rule excludes {100 * xc:.2f} % / {100 * xa:.2f} % of {c['N']} tokens (caption / acoustic gate)")
    r0 = run_gate(lib, c, 0, True, True)
    assert bool(torch.isfinite(r0["lc"]).all())
    within(f"caption_gate form 0 T={T} logits", r0["lc"], ref["lc"], ref["lc_bound"])
    check_gate(f"caption_gate form 0 T={T}", c, ref, r0, True, r0["lc"])
    r1 = run_gate(lib, c, 1, True, True)
    same_decisions(f"form 1 vs form 0, injected noise, T={T}", r1, r0)
    check_gate(f"caption_gate form 1 T={T}", c, ref, r1, True, r0["lc"])
    same_decisions(f"form 0 without lc_out, T={T}", run_gate(lib, c, 0, True, True, want_lc=False), r0)
    d0, d1 = run_gate(lib, c, 0, False, False), run_gate(lib, c, 1, False, False)
    same_decisions(f"form 1 vs form 0, device-drawn noise, T={T}", d1, d0)
    assert int(d0["ic"].min()) >= 0 and int(d0["ic"].max()) < 4 and bool(torch.isfinite(d0["mc"]).all())
    assert torch.equal(d0["cnt"].long(), O.count_table(d0["ic"], d0["ia"], 4, False)), "count table per expert group, device-drawn noise"
    assert torch.equal(d0["lc"].view(torch.int32), r0["lc"].view(torch.int32)), "the logits do not depend on the noise"


def test_caption_gate_eight_experts_on_the_router_form(lib):
    """E = 8 takes the router's run-time-bound instance; the one-launch kernel refuses it"""
    c, ref = gate_case(130, 8)
    xc, xa = O.excluded_share(ref)
    assert xc <= O.MARGIN_CAP and xa <= O.MARGIN_CAP
    r0 = run_gate(lib, c, 0, True, False)
    assert bool(torch.isfinite(r0["lc"]).all())
    within("caption_gate form 0 E=8 logits", r0["lc"], ref["lc"], ref["lc_bound"])
    check_gate("caption_gate form 0 E=8", c, ref, r0, False, r0["lc"])
    with pytest.raises(L.VersbandError, match="form 1 does not support"):
        run_gate(lib, c, 1, True, False)


def test_unit_wrappers_refuse_null_pointers_and_empty_sizes(lib):
    one = torch.zeros(64, device="cuda")
    p, s = L.ptr(one), L.stream_ptr()
    assert lib.vb_band_ffn(None, 200, p, p, 1, 64, 1, 192, p, 192, 1, p, 192, s) == -1
    assert lib.vb_band_ffn(p, 200, p, p, 0, 64, 1, 192, p, 192, 1, p, 192, s) == -1
    assert lib.vb_band_ffn(p, 576, p, p, 1, 64, 3, 192, p, 576, 1, p, 576, s) == -1 and b"E=3 unsupported" in lib.vb_last_error()
    assert lib.vb_routed_ffn_pair(p, p, p, p, p, p, p, p, None, 1, 16, 64, 1, p, p, s) == -1
    assert lib.vb_routed_ffn_pair(p, p, p, p, p, p, p, p, p, 0, 16, 64, 1, p, p, s) == -1
    assert lib.vb_caption_gate(p, p, p, p, p, p, 1, p, 2, None, None, None, 0, 0, 0, 0, 1, 1, 0, 768, 640, 8, 4, 0, p, p, p, p, p, p, None, None, 0, 0, s) == -1
    assert lib.vb_caption_gate(p, p, p, p, p, p, 1, p, 2, p, None, None, 0, 0, 0, 0, 1, 1, 1, 768, 640, 8, 4, 0, p, p, p, p, p, p, None, None, 0, 0, s) == -1
    torch.cuda.synchronize()
