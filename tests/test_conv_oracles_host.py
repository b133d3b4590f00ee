"""The conv oracles of tests/conv_oracles.py judged without a GPU: (a) an fp32 emulation of each kernel family's arithmetic stays inside the
derived bound at every shape of tests/test_gpu_conv_units.py, (b) float64 results on WRONG operands - the faults a conv kernel can have at
its edges - leave the bound by at least FACTOR on their designated (clip, position) columns, (c) every GPU case is planned on the host
(vb_conv1d_plan / vb_respair_plan need no device) as the kernel and tile it was written for.  Each test prints its worst err / bound or
its smallest rejection factor (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_oracles as O
from versband_amd import _lib as L

FACTOR = 2.0
IDS = [c["id"] for c in O.CASES]
PAIR_IDS = [c["id"] for c in O.PAIR_CASES]
_WORST = {}


def inside(what, fam, got, ref, bound):
    assert bool(torch.isfinite(ref).all()) and bool((bound > 0).all()), what
    err = (got.double() - ref).abs()
    r = O.worst(err, bound)
    _WORST[fam] = max(_WORST.get(fam, 0.0), r)
    print(f"{what}: worst err / bound = {r:.3f}   (family so far {_WORST[fam]:.3f})")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements of a correct fp32 evaluation outside the bound"


# ------------------------------------------------------------------------------------------------------------------ (a) emulation
@pytest.mark.parametrize("c", O.CASES, ids=IDS)
def test_conv_bound_holds_for_the_fp32_emulation(c):
    inp = O.conv_inputs(c)
    ref, bound = O.conv_reference(c, inp)
    if c["fam"] == "mf":
        assert c["mf_disagreement"] <= 1e-12, f"{c['id']}: pseudo-tap algebra and plain convolution differ by {c['mf_disagreement']:.3g} S"
    inside(c["id"], c["fam"], O.conv_emulation(c, inp), ref, bound)


@pytest.mark.parametrize("c", O.PAIR_CASES, ids=PAIR_IDS)
def test_pair_bound_holds_for_the_fp32_emulation(c):
    inp = O.pair_inputs(c)
    ref, bound = O.pair_reference(c, inp)
    if c["fam"] == "mf":
        assert c["mf_disagreement"] <= 1e-12, f"{c['id']}: pseudo-tap algebra and plain convolution differ by {c['mf_disagreement']:.3g} S"
    inside(c["id"], "pair-" + c["fam"], O.pair_emulation(c, inp), ref, bound)


# ------------------------------------------------------------------------------------------------------------------ (b) wrong results
def factor(what, wrong, ref, bound, cols, clips=None):
    """smallest over the designated (clip, position) columns of the largest err / bound over the channels; asserted >= FACTOR"""
    r = ((wrong - ref).abs() / bound).amax(1)            # [B][T_out]
    r = r[:, cols] if clips is None else r[clips][:, cols]
    assert r.numel(), f"{what}: no designated column"
    f = float(r.min())
    assert f >= FACTOR, f"{what}: leaves the bound by {f:.2f}x only on a designated column (need {FACTOR:g}x)"
    return f


def _wrong(c, inp, xo=None, wo=None, res=None, out_in=None, dil=None, conv=None, ep=None):
    """the reference pipeline on mutated operands (float64; the minimal-filtering family through the plain convolution it equals)"""
    x0, w0 = O.operands(c, inp)
    xo, wo = x0 if xo is None else xo, w0 if wo is None else wo
    cc = dict(c, dil=dil) if dil is not None else c
    a = conv(xo, wo) if conv else O.raw_conv(cc, xo, wo)
    if ep:
        return ep(a)
    return O.epilogue(a, torch.zeros_like(a), inp["b"], inp["res"] if res is None else res, inp["out_in"] if out_in is None else out_in,
                      c["alpha"], c["beta"])[0]


def _padded_conv(c, xp, wo):
    """ordinary convolution of an explicitly padded image"""
    return F.conv1d(xp, wo, dilation=c["dil"])[..., :c["T_out"]]


def conv_mutations(c, inp):
    """(name, wrong, designated columns, designated clips or None) of every listed fault this case can show"""
    xo, wo = O.operands(c, inp)
    B, Ci, Te = xo.shape
    k, dil, pad, To = c["ntaps"], c["dil"], c["pad"], c["T_out"]
    plain = not c["tr"]
    # a fault that shifts or drops operands everywhere is judged where a single column cannot hide it by chance: the columns whose taps
    # all read inside the clip, at both ends and in the middle, of the clips that are not the quiet one
    inner = [t for t in range(To) if t - pad >= 0 and t - pad + (k - 1) * dil < Te] if plain else list(range(To))
    every = sorted({inner[i] for i in (0, 1, len(inner) // 2, -2, -1)}) if len(inner) >= 2 else inner
    loud = list(range(B - 1)) if B >= 2 else None
    anyc = every or [t for t in sorted({0, To // 2, To - 1}) if any(0 <= t - pad + j * dil < Te for j in range(k))]
    out = []
    if plain and k > 1:
        t = Te - 1 + pad - (k - 1) * dil          # the output whose last tap reads the clip's last column
        if 0 <= t < To:
            w1 = wo.clone(); w1[..., k - 1] = 0
            out.append(("last tap dropped at the right clip edge", _wrong(c, inp, wo=w1), [t], None))
        if pad >= 1 and pad - 1 < To:
            padr = max(0, (To - 1) - pad + (k - 1) * dil - (Te - 1))
            xp = F.pad(xo, (pad, padr))
            if B >= 2:
                xq = xp.clone(); xq[1:, :, pad - 1] = xo[:-1, :, -1]
                out.append(("first pad column read from the neighbouring clip", _wrong(c, inp, conv=lambda x, w: _padded_conv(c, xq, w)), [pad - 1], list(range(1, B))))
            xq = xp.clone(); xq[:, 1:, pad - 1] = xo[:, :-1, -1]
            out.append(("first pad column read from the neighbouring channel row", _wrong(c, inp, conv=lambda x, w: _padded_conv(c, xq, w)), [pad - 1], None))
        if Te >= 2 and every:
            xs = F.pad(xo, (1, 0))[..., :-1]
            out.append(("padding off by one", _wrong(c, inp, xo=xs), every, loud))
            wide = F.conv1d(F.pad(xo, (pad, pad + k)), wo, dilation=dil + 1)
            if wide.shape[-1] >= To:
                out.append(("dilation off by one", _wrong(c, inp, conv=lambda x, w: wide[..., :To]), every, loud))
        if c["halo"] == 64:
            w1 = wo.clone(); w1[..., [j for j in range(k) if j * dil > 60]] = 0
            cols = [t for t in range(To) if any(j * dil > 60 and 0 <= t - pad + j * dil < Te for j in range(k))]
            out.append(("halo truncated to 60", _wrong(c, inp, wo=w1), cols, None))
    # (a bf16 copy errs by ~UB / 2 per value, ~0.3 UB sqrt(K) S / K summed; the bound is 2 K U32 S: the ratio 2^14 * 0.3 / K^1.5 is above
    #  4 up to K = Ci taps = 112, so the fault is designated at those shapes - the narrow-K cases of every fp32 route)
    if c["fam"] in ("f32", "mf") and plain and c["halo"] >= 1 and Ci * k <= 112:
        h = min(c["halo"], Te)
        xb = xo.clone(); xb[..., :h] = O.bf16r(xo[..., :h]); xb[..., -h:] = O.bf16r(xo[..., -h:])
        tl = Te - 1 + pad - (k - 1) * dil
        out.append(("halo columns taken from a bf16 copy", _wrong(c, inp, xo=xb), [0] + ([tl] if 0 < tl < To else []), None))
    if c["fam"] in ("x3", "x3xt") and plain:
        tile = c["plan"][2]
        cols = list(range((To - 1) // tile * tile, To))
        out.append(("lo plane dropped on the last tile's columns", _wrong(c, inp, xo=O.split(O.activated(c, inp["x"]))[0]), cols, None))
    if Ci > 16:
        xz = xo.clone(); xz[:, (Ci - 1) // 16 * 16:] = 0
        out.append(("last channel chunk skipped", _wrong(c, inp, xo=xz), anyc, loud))
    if c["tr"]:
        out.append(("transposed conv with phase p + 1's weights", _wrong(c, inp, wo=torch.roll(wo, 1, -1)), every, loud))
        out.append(("transposed conv with phase p - 1's weights", _wrong(c, inp, wo=torch.roll(wo, -1, -1)), every, loud))
    if c["ups"] and Te >= 4:
        out.append(("upsample2 reading x[t / 2 + 1]", _wrong(c, inp, xo=torch.roll(xo, -2, -1)), [t for t in every if t < To - 2], loud))
        out.append(("upsample2 reading x[t / 2 - 1]", _wrong(c, inp, xo=torch.roll(xo, 2, -1)), [t for t in every if t >= 2], loud))
    if c["res"] and c["alpha"] != 1.0:
        def unscaled(a):
            r0 = O.epilogue(a, torch.zeros_like(a), inp["b"], None, inp["out_in"], c["alpha"], c["beta"])[0]
            return r0 + inp["res"].double()
        out.append(("residual not scaled by alpha", _wrong(c, inp, ep=unscaled), anyc, loud))
    if c["beta"] != 0.0 and To >= 2:
        out.append(("beta applied to the neighbouring element", _wrong(c, inp, out_in=torch.roll(inp["out_in"], 1, -1)), anyc, loud))
    return out


@pytest.mark.parametrize("c", O.CASES, ids=IDS)
def test_conv_bound_rejects_wrong_results(c):
    inp = O.conv_inputs(c)
    ref, bound = O.conv_reference(c, inp)
    muts = conv_mutations(c, inp)
    fs = {name: factor(f"{c['id']}: {name}", wrong, ref, bound, cols, clips) for name, wrong, cols, clips in muts}
    key = c["fam"]
    if fs:
        _WORST["rej-" + key] = min(_WORST.get("rej-" + key, float("inf")), min(fs.values()))
        print(f"{c['id']}: {len(fs)} wrong results, smallest rejection factor {min(fs.values()):.3g} ({min(fs, key=fs.get)}); family so far {_WORST['rej-' + key]:.3g}")


def test_every_listed_fault_is_shown_by_some_case():
    """the case table keeps a shape for every fault of the list (a retune of the table cannot silently drop one)"""
    seen = set()
    for c in O.CASES:
        if c["B"] * c["Co"] * c["T_out"] > 200000:
            continue
        seen |= {m[0] for m in conv_mutations(c, O.conv_inputs(c))}
    assert len(seen) == 15, sorted(seen)


def pair_wrong(c, inp, mode):
    """the pair's float64 chain with one fault; -> (wrong, designated columns)"""
    k, dil, T = c["k"], c["dil"], c["T"]
    h2 = (k - 1) // 2
    cc = dict(c, fam={"mf": "f32"}.get(c["fam"], c["fam"]))          # (plain convolution: equal to the pseudo-tap algebra in float64)
    x = inp["x"]
    xa = O.lrelu32(x)
    if mode == "unzeroed":      # the intermediate keeps conv1's values outside [0, T)
        xa = F.pad(xa, (h2, h2))
    a1, _, _ = O._pair_stage(cc, xa, inp["w1"], dil)
    v1 = a1 + inp["b1"].double().view(1, -1, 1)
    h = torch.where(v1 > 0, v1, v1 * float(O.np.float32(O.SLOPE)))
    if c["fam"] == "bf16":
        h = O.bf16r(h)
    wo = (sum(O.split(inp["w2"])) if c["fam"] == "x3" else O.bf16r(inp["w2"].double()) if c["fam"] == "bf16" else inp["w2"].double())
    cols = [0, T - 1]
    if mode == "unzeroed":
        a2 = F.conv1d(h, wo)
    else:
        if mode == "short":          # T taken one short: the last intermediate column is padding
            h = h.clone(); h[..., -1] = 0
            cols = [T - 1]
        elif mode == "long":         # T taken one long: conv2 reads conv1's value at position T
            xl = F.pad(xa, (0, 1))
            hl = O._pair_stage(cc, xl, inp["w1"], dil)[0] + inp["b1"].double().view(1, -1, 1)
            hl = torch.where(hl > 0, hl, hl * float(O.np.float32(O.SLOPE)))
            a2 = F.conv1d(F.pad(hl, (h2, h2 - 1)), wo)
            cols = [T - 1]
        elif mode == "stale":        # the second workgroup's left conv2 halo holds the previous clip's columns
            n0 = c["outputs"]
            h = h.clone(); h[:, :, n0 - h2:n0] = torch.roll(h, 1, 0)[:, :, n0 - h2:n0]
            cols = [n0]
        if mode != "long":
            a2 = F.conv1d(h, wo, padding=h2)
    return O.epilogue(a2, torch.zeros_like(a2), inp["b2"], x, inp["out_in"], c["alpha"], c["beta"])[0], cols


@pytest.mark.parametrize("c", O.PAIR_CASES, ids=PAIR_IDS)
def test_pair_bound_rejects_wrong_results(c):
    inp = O.pair_inputs(c)
    ref, bound = O.pair_reference(c, inp)
    c = dict(c, outputs=O.pair_plan(L.load(), c)[1])
    modes = ["unzeroed", "short", "long"] + (["stale"] if c["T"] > c["outputs"] else [])
    fs = {}
    for mode in modes:
        if c["T"] == 1 and mode != "unzeroed":
            continue
        wrong, cols = pair_wrong(c, inp, mode)
        fs[mode] = factor(f"{c['id']}: {mode}", wrong, ref, bound, cols)
    key = "rej-pair-" + c["fam"]
    _WORST[key] = min(_WORST.get(key, float("inf")), min(fs.values()))
    print(f"{c['id']}: smallest rejection factor {min(fs.values()):.3g} ({min(fs, key=fs.get)}); family so far {_WORST[key]:.3g}")


# ------------------------------------------------------------------------------------------------------------------ (c) plans on the host
@pytest.mark.parametrize("c", O.CASES, ids=IDS)
def test_every_gpu_case_is_planned_as_the_kernel_it_was_written_for(c):
    lib = L.load()
    try:
        L.set_tuning(**c["knobs"])
        O.assert_plan(lib, c)
    finally:
        L.set_tuning(**{k: None for k in c["knobs"]})


def test_plan_follows_the_knobs_and_refuses_what_the_launch_refuses():
    lib = L.load()
    c = next(c for c in O.CASES if c["plan"][0] == O.F32G)
    w = next(c for c in O.CASES if c["plan"][0] == O.F32W)
    try:
        L.set_tuning(VB_CONV_F32_OLD="1")
        assert O.conv_plan(lib, c)[0] == O.F32
        L.set_tuning(VB_CONV_F32_OLD=None, VB_CONV_MF_OFF="1")
        assert O.conv_plan(lib, w)[0] == O.F32G
        L.set_tuning(VB_CONV_MF_OFF=None, VB_CONV_DIRECT_EPI="1")
        assert O.conv_plan(lib, w)[0] == O.F32G and O.conv_plan(lib, w)[3] == 0      # no minimal filtering without the staged epilogue
    finally:
        L.set_tuning(VB_CONV_F32_OLD=None, VB_CONV_MF_OFF=None, VB_CONV_DIRECT_EPI=None)
    assert O.conv_plan(lib, w)[0] == O.F32W
    import ctypes as C
    r = [C.c_int() for _ in range(4)]
    assert lib.vb_conv1d_plan(2, 16, 64, 64, 3, 33, 33, 1, 0, 0, 64, 0, 1, 0, 0, 32, 1.0, 0.0, 1, 0, 0, 0, 0, *[C.byref(v) for v in r]) != 0      # halo 66
    assert lib.vb_respair_plan(O.PAIR_F32, 2, 32, 62, 3, 1, 0, *[C.byref(v) for v in r]) != 0                                                    # T % 4
    assert lib.vb_respair_plan(O.PAIR_MF, 2, 128, 64, 3, 1, 0, *[C.byref(v) for v in r]) != 0                                                    # C = 128


@pytest.mark.parametrize("c", O.PAIR_CASES, ids=PAIR_IDS)
def test_pair_cases_cover_their_run_boundaries(c):
    run, outputs, grid_t, staged = O.pair_plan(L.load(), c)
    assert outputs == (run - (c["k"] - 1)) // 4 * 4 and grid_t == -(-c["T"] // outputs)
    assert staged == (c["T"] % 4 == 0)
