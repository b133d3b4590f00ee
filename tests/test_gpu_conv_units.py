"""Every convolution kernel and ResBlock-pair kernel alone behind its C-ABI unit wrapper, against the float64 oracles of tests/conv_oracles.py
and their derived per-element bounds, at the kernels' own edges (the case table lives in conv_oracles.py, the host tests run the same
shapes).  Each case first asserts its plan (vb_conv1d_plan / vb_respair_plan): a case that no longer reaches the kernel and tile it was
written for fails.  Outputs, residuals and beta operands live inside larger device buffers behind a 256-float guard band of a fixed bit
pattern on both sides (an interior pointer, 16-byte or - where the route allows - only 4-byte aligned), the input between large finite
guards (2^14): after the launch every guard keeps its bits, every output is finite and inside its bound, nothing excluded.  Each case
prints its worst err / bound (pytest -s)."""
import ctypes as C

import pytest
import torch

from tests import conv_oracles as O
from versband_amd import _lib as L
from versband_amd import pack

pytestmark = pytest.mark.gpu
GUARD = 256
PATTERN = 0x7FC5A5A5        # guard bits of the float buffers (a NaN no kernel writes)
BIG = 2.0 ** 14
_WORST = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


class Guarded:
    """t inside a larger device buffer: [GUARD | (one float when four_byte) | t | GUARD], the bands holding `fill` bits or the value `big`"""

    def __init__(self, t, four_byte=False, big=None):
        n, off = t.numel(), GUARD + (1 if four_byte else 0)
        flat = torch.empty(off + n + GUARD, dtype=torch.float32)
        if big is None:
            flat.view(torch.int32).fill_(PATTERN)
        else:
            flat.fill_(big)
        self.band = flat.clone().view(torch.int32)
        flat[off:off + n] = t.reshape(-1).float()
        self.flat, self.off, self.n, self.shape = flat.cuda(), off, n, t.shape
        assert self.flat.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.flat.data_ptr() + 4 * self.off)

    def value(self):
        return self.flat[self.off:self.off + self.n].view(self.shape).cpu()

    def intact(self):
        got = self.flat.cpu().view(torch.int32)
        return bool((got[:self.off] == self.band[:self.off]).all()) and bool((got[self.off + self.n:] == self.band[self.off + self.n:]).all())


def dev(t):
    return t.contiguous().cuda()


def launch_conv(lib, c, inp):
    """-> (output fp32 [B][Co][T_out] on the host, the guarded buffers)"""
    B, Ci, T, Co, To = c["B"], c["Ci"], c["T"], c["Co"], c["T_out"]
    x = Guarded(inp["x"], c["mis"] & O.X_4B, big=BIG)
    out = Guarded(inp["out_in"] if inp["out_in"] is not None else torch.full((B, Co, To), float("nan")), c["mis"] & O.OUT_4B)
    res = Guarded(inp["res"], c["mis"] & O.RES_4B) if inp["res"] is not None else None
    b = dev(inp["b"])
    wpk = pack.pack_conv_transpose(inp["w"], c["u"]) if c["tr"] else pack.pack_conv(inp["w"])
    rp = res.ptr if res else None
    keep = [b]
    if c["fam"] == "f32" and c["ups"]:
        wd = dev(wpk)
        keep.append(wd)
        assert c["alpha"] == 1.0 and c["beta"] == 0.0 and not c["tr"] and c["stride"] == 1
        L.check(lib.vb_conv1d_f32_ups(x.ptr, L.ptr(wd), L.ptr(b), B, Ci, T, Co, c["k"], c["dil"], c["pad"], To, c["act"], O.SLOPE, rp, out.ptr,
                                      L.stream_ptr()), c["id"])
    elif c["fam"] == "x3xt":
        wx, cip = pack.pack_conv_x3(wpk)
        wx = dev(wx)
        scratch = torch.empty(lib.vb_xt_planes_bytes(B, Ci, T, c["ups"], 2) + 16, dtype=torch.uint8, device="cuda")
        keep += [wx, scratch]
        L.check(lib.vb_conv1d_x3_xt(x.ptr, L.ptr(wx), cip, L.ptr(b), B, Ci, T, Co, c["k"], c["dil"], c["pad"], To, c["ups"], c["act"], O.SLOPE, rp,
                                    c["alpha"], c["beta"], out.ptr, L.ptr(scratch), L.stream_ptr()), c["id"])
    elif c["fam"] in ("f32", "x3"):
        wd = dev(wpk)
        wx, cip = pack.pack_conv_x3(wpk) if c["fam"] == "x3" else (None, 0)
        wx = dev(wx) if wx is not None else None
        keep += [wd, wx]
        assert c["alpha"] == 1.0 and c["beta"] == 0.0 and not c["ups"] and c["stride"] == 1
        L.check(lib.vb_conv1d_f32(x.ptr, L.ptr(wd), L.ptr(b), B, Ci, T, Co, c["k"], c["dil"], c["pad"], c["u"], c["tr_pad"], c["tr_k"], To,
                                  c["act"], O.SLOPE, rp, out.ptr, L.ptr(wx), cip, L.stream_ptr()), c["id"])
    elif c["fam"] == "mf":
        wd, wm = dev(wpk), dev(pack.pack_conv_mf(inp["w"]))
        keep += [wd, wm]
        L.check(lib.vb_conv1d_f32_mf(x.ptr, L.ptr(wd), L.ptr(wm), L.ptr(b), B, Ci, T, Co, c["k"], c["dil"], c["pad"], To, c["act"], O.SLOPE, rp,
                                     c["alpha"], c["beta"], out.ptr, L.stream_ptr()), c["id"])
    else:
        wb, cip = pack.pack_conv_bf16(wpk)
        wb = dev(wb)
        keep.append(wb)
        gn = [dev(inp[n]) for n in ("mean", "rstd", "gamma", "gbeta")] if c["gn"] else [None] * 4
        keep += gn
        args = [x.ptr, L.ptr(wb), cip, L.ptr(b), B, Ci, T, Co, c["k"], c["dil"], c["pad"], c["u"], c["tr_pad"], c["tr_k"], To, c["ups"], c["stride"],
                c["phase"], c["act"], O.SLOPE, *[L.ptr(g) for g in gn], c["gn"][0] if c["gn"] else 0, rp, c["alpha"], c["beta"], out.ptr]
        if c["fam"] == "bf16xt":
            scratch = torch.empty(lib.vb_conv1d_bf16_xt_scratch_bytes(B, Ci, T, c["ups"]) + 16, dtype=torch.uint8, device="cuda")
            keep.append(scratch)
            L.check(lib.vb_conv1d_bf16_xt(*args, L.ptr(scratch), L.stream_ptr()), c["id"])
        else:
            L.check(lib.vb_conv1d_bf16(*args, L.stream_ptr()), c["id"])
    torch.cuda.synchronize()
    del keep
    return out.value(), [g for g in (x, out, res) if g is not None]


def judge(what, fam, got, ref, bound, bufs):
    for g in bufs:
        assert g.intact(), f"{what}: a guard band around a buffer of {g.n} floats was written"
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} outputs not finite (never written, or a guard value read)"
    err = (got.double() - ref).abs()
    r = O.worst(err, bound)
    _WORST[fam] = max(_WORST.get(fam, 0.0), r)
    print(f"{what}: worst err / bound = {r:.3f}   (family so far {_WORST[fam]:.3f})")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst {r:.2f}x"


# the A/B switches that select between builds documented as bit-identical, per planned route (a case runs them when its output is small).
# The conv-mode GEMM has two tiles, 64 x 64 and 128 x 128, chosen by workgroup count alone (gemm_route's last rule: VB_GEMM_TILE does not
# reach it); VB_GEMM_SMALL=0 keeps 128 x 128.  Where a switch shows in the plan - another route, tile or epilogue - the plan under it
# must differ from the default's, so that a switch that stopped switching does not compare a build with itself; VB_CONV_F32_RT_TAPS and
# VB_MF_OCC select instances of one route and tile, which the plan does not name.
SAME_BITS = {O.F32G: [{"VB_CONV_F32_OLD": "1"}, {"VB_CONV_F32_RT_TAPS": "1"}, {"VB_CONV_DIRECT_EPI": "1"}], O.F32W: [{"VB_MF_OCC": "3"}],
             O.X3: [{"VB_CONV_DIRECT_EPI": "1"}], O.BF16: [{"VB_CONV_DIRECT_EPI": "1"}], O.BF16_XT: [{"VB_CONV_DIRECT_EPI": "1"}],
             O.X3_XT: [{"VB_CONV_DIRECT_EPI": "1"}], O.CO1: [{"VB_CONV_F32_OLD": "1"}], O.AS_GEMM: [{"VB_GEMM_SMALL": "0"}]}
IN_PLAN = ("VB_CONV_F32_OLD", "VB_GEMM_SMALL")


@pytest.mark.parametrize("c", O.CASES, ids=[c["id"] for c in O.CASES])
def test_conv_unit_inside_its_bound(lib, c):
    inp = O.conv_inputs(c)
    ref, bound = O.conv_reference(c, inp)
    try:
        L.set_tuning(**c["knobs"])
        plan = O.assert_plan(lib, c)
        got, bufs = launch_conv(lib, c, inp)
    finally:
        L.set_tuning(**{k: None for k in c["knobs"]})
    judge(c["id"], c["fam"], got, ref, bound, bufs)
    if c["knobs"] or got.numel() > 100000:
        return
    for knobs in SAME_BITS.get(c["plan"][0], []):
        try:
            L.set_tuning(**knobs)
            if any(k in IN_PLAN for k in knobs) or ("VB_CONV_DIRECT_EPI" in knobs and plan[3]):
                assert O.conv_plan(lib, c) != plan, f"{c['id']}: {knobs} leaves the plan at {plan}"
            alt, bufs = launch_conv(lib, c, inp)
        finally:
            L.set_tuning(**{k: None for k in knobs})
        assert all(g.intact() for g in bufs), f"{c['id']} {knobs}: a guard band was written"
        assert torch.equal(alt, got), f"{c['id']}: {knobs} changes {int((alt != got).sum())} of {got.numel()} outputs (documented as bit-identical)"


GPU_PAIRS = O.PAIR_CASES


@pytest.mark.parametrize("c", GPU_PAIRS, ids=[c["id"] for c in GPU_PAIRS])
def test_pair_unit_inside_its_bound(lib, c):
    inp = O.pair_inputs(c)
    ref, bound = O.pair_reference(c, inp)
    B, Cc, T, k = c["B"], c["C"], c["T"], c["k"]
    run, outputs, grid_t, staged = O.pair_plan(lib, c)
    assert outputs == (run - (k - 1)) // 4 * 4 and grid_t == -(-T // outputs) and staged == (T % 4 == 0), (c["id"], run, outputs, grid_t, staged)
    pk = {O.PAIR_F32: pack.pack_conv, O.PAIR_MF: pack.pack_conv_mf, O.PAIR_BF16: lambda w: pack.pack_conv_bf16(pack.pack_conv(w))[0],
          O.PAIR_X3: lambda w: pack.pack_conv_x3(pack.pack_conv(w))[0]}[c["form"]]
    fn = {O.PAIR_F32: lib.vb_respair_f32, O.PAIR_MF: lib.vb_respair_f32_mf, O.PAIR_BF16: lib.vb_respair_bf16, O.PAIR_X3: lib.vb_respair_x3}[c["form"]]
    w1, w2, b1, b2 = dev(pk(inp["w1"])), dev(pk(inp["w2"])), dev(inp["b1"]), dev(inp["b2"])

    def launch():
        x = Guarded(inp["x"], big=BIG)
        out = Guarded(inp["out_in"] if inp["out_in"] is not None else torch.full((B, Cc, T), float("nan")))
        L.check(fn(x.ptr, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), B, Cc, T, k, c["dil"], O.SLOPE, c["alpha"], c["beta"], out.ptr, L.stream_ptr()), c["id"])
        torch.cuda.synchronize()
        return out.value(), [x, out]
    got, bufs = launch()
    judge(c["id"], "pair-" + c["fam"], got, ref, bound, bufs)
    for knobs in ([{"VB_CONV_DIRECT_EPI": "1"}, {"VB_CONV_F32_RT_TAPS": "1"}] if c["form"] == O.PAIR_F32 else [{"VB_CONV_DIRECT_EPI": "1"}] if c["form"] in (O.PAIR_BF16, O.PAIR_X3) else []):
        try:
            L.set_tuning(**knobs)
            alt, bufs = launch()
        finally:
            L.set_tuning(**{k_: None for k_ in knobs})
        assert all(g.intact() for g in bufs), f"{c['id']} {knobs}: a guard band was written"
        assert torch.equal(alt, got), f"{c['id']}: {knobs} changes {int((alt != got).sum())} of {got.numel()} outputs (documented as bit-identical)"
