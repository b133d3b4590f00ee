"""Window rows on the GPU (vb_sample_cfg_window_rows, vb_window_rows_blend, through the C ABI): joint windows of long clips of DIFFERENT
lengths as rows of one sampler call - a per-row plan (group, start) beside the row lengths, and after every Euler step the overlapping
tokens of neighbouring rows of a group take one consensus value m = fmaf(g, x[ib] - x[ia], x[ia]), g = (u + 1) / (ov + 1).

The mixed call: 11 rows at T = 40, five long clips, their rows interleaved in the row order (A0 B0 A1 C0 B1 D0 E0 A2 D1 E1 E2):
  A 100 tokens  (0,40) (32,40) (60,40)   overlaps 8 and 12, a shifted last window
  B  70 tokens  (0,40) (30,40)           other starts, another window count
  C  25 tokens  (0,25)                   a single short row, no pair
  D  49 tokens  (0,40) (32,17)           an overlap of 8 that ends inside a short row
  E  56 tokens  (0,40) (32,16) (40,16)   a middle row whose two overlaps fill it exactly (8 + 8 = 16): the three-row bound met with equality

Bounds.  The blend unit is compared with a float64 restatement that forms d = float32(xb - xa) and g = float32(u + 1) / float32(ov + 1) in
fp32 first, at 2e-7 of max-abs (derived in tests/test_gpu_joint.py: one fma rounding against a float64 and an fp32 rounding, at most 1 ulp
of |m| <= max-abs).  Group D's trajectory is compared with a CPU restatement over oracle.ref_cpu.dit_forward on each row's own tokens at
the project's 3-step CFG-trajectory bound, rel-L2 1e-3 (the blend is a convex combination and does not widen it), with equal routing
indices.  A kept token is compared with the host's r(t) at 2e-7 of max-abs, as tests/test_gpu_keep.py does.  Everything that claims "the
same bits" is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, clip_batch, describe, exp_noise, gumbel_arrays, gumbel_arrays_steps, rel_l2
from versband_amd import _lib as L
from versband_amd import longform
from versband_amd import model as vm
from versband_amd import prng, synth

pytestmark = pytest.mark.gpu
SIGMA = 1e-4            # CFM.sigma_min (versband_amd/model.py)
ALL_ONE = 2e-7          # of the tensor's max-abs
T, LC, NCH = 40, 8, 20
CLIP_LEN = {"A": 100, "B": 70, "C": 25, "D": 49, "E": 56}
GROUPS = {"A": [(0, 40), (32, 40), (60, 40)], "B": [(0, 40), (30, 40)], "C": [(0, 25)], "D": [(0, 40), (32, 17)], "E": [(0, 40), (32, 16), (40, 16)]}
ORDER = [("A", 0), ("B", 0), ("A", 1), ("C", 0), ("B", 1), ("D", 0), ("E", 0), ("A", 2), ("D", 1), ("E", 1), ("E", 2)]
VB_E_INVALID = -1


def _gid(g):
    return "ABCDE".index(g)


def _key(g, w):
    """the global clip id a row draws its router noise under: fixed per (group, window), whatever call the row rides in"""
    return 10 * _gid(g) + w + 3


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Context("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(synth.dit_shapes(synth.DiTConfig()), SEED)


@pytest.fixture(scope="module")
def engines(ctx, sd):
    from versband_amd.engine import DiTEngine
    return {prec: DiTEngine(ctx, synth.DiTConfig(), sd, precision=prec) for prec in ("split", "bf16")}


def _fresh(ctx, sd, engines, prec="bf16"):
    """an engine with its own context (its own graph cache) on the shared packed weights"""
    from versband_amd.engine import DiTEngine
    return DiTEngine(ctx, synth.DiTConfig(), sd, precision=prec, share=engines[prec])


@pytest.fixture
def knobs(monkeypatch):
    names = []

    def set_(**kw):
        for k in names:
            monkeypatch.delenv(k, raising=False)
        names.clear()
        for k, v in kw.items():
            monkeypatch.setenv(k, v)
            names.append(k)
        L.load().vb_tune_reload()
    yield set_
    set_()


def _rnd(shape, name, scale=1.0):
    return torch.from_numpy(prng.normal(prng.key_seed(17, name), int(np.prod(shape))).reshape(shape)).float() * scale


@pytest.fixture(scope="module")
def clips():
    """the five long clips, each with a long known-region reference of its own"""
    out = {g: synth.make_clip_inputs(SEED, _gid(g), n, L=LC) for g, n in CLIP_LEN.items()}
    for g, n in CLIP_LEN.items():
        out[g]["ref"] = _rnd((NCH, n), f"ref{g}")
    return out


def _call(clips, order=ORDER, pad_x=None, pad_track=0):
    """the rows of a call: every (group, window) of `order` cut out of its long clip and padded to T (x with finite noise, or pad_x; midi
    with pad_track, beats with 1 beside a non-zero pad_track), the plan and the rows' noise keys"""
    R = len(order)
    x = _rnd((R, NCH, T), "xpad", 0.5) if pad_x is None else torch.full((R, NCH, T), float(pad_x))
    ref = torch.zeros(R, NCH, T)
    midi = torch.full((R, 2 * T), pad_track, dtype=torch.int64)
    beats = torch.full((R, 2 * T), 1 if pad_track else 0, dtype=torch.int64)
    for r, (g, w) in enumerate(order):
        s, m = GROUPS[g][w]
        x[r, :, :m] = clips[g]["x_latent"][:, s:s + m]
        ref[r, :, :m] = clips[g]["ref"][:, s:s + m]
        midi[r, :2 * m] = clips[g]["midi"][0, 2 * s:2 * (s + m)]
        beats[r, :2 * m] = clips[g]["beats"][0, 2 * s:2 * (s + m)]
    tc = torch.stack([clips[g]["t5_cond"] for g, _ in order])
    tu = torch.stack([clips[g]["t5_uncond"] for g, _ in order])
    return dict(x=x, ref=ref, midi=midi, beats=beats, tc=tc, tu=tu, t5=torch.cat([tc, tu]), group=[_gid(g) for g, _ in order],
                start=[GROUPS[g][w][0] for g, w in order], lens=[GROUPS[g][w][1] for g, w in order], keys=[_key(g, w) for g, w in order],
                order=list(order))


def _pairs(c):
    """[(ra, rb, off_a, ov)] of a call: consecutive rows of a group"""
    last, out = {}, []
    for r, g in enumerate(c["group"]):
        if g in last:
            ra = last[g]
            ov = c["start"][ra] + c["lens"][ra] - c["start"][r]
            if ov > 0:
                out.append((ra, r, c["lens"][ra] - ov, ov))
        last[g] = r
    return out


def _sample(eng, c, idx, dts, scale=3.0, seed=5, **kw):
    cond = eng.precompute_cond(c["t5"], c["midi"], c["beats"], T, lengths=c["lens"])
    return eng.sample_cfg(c["x"], cond, idx, dts, scale, seed=seed, clip_ids=c["keys"], window_rows=(c["group"], c["start"]), lengths=c["lens"], **kw)


def _assert_overlaps_agree(x, c, what):
    for ra, rb, off, ov in _pairs(c):
        a, b = x[ra, :, off:off + ov], x[rb, :, :ov]
        assert torch.equal(a, b), describe(f"{what}: overlap of rows {ra} / {rb} ({ov} tokens)", a, b)


def _blend_torch(x, c):
    """the consensus written in torch, in x's dtype"""
    x = x.clone()
    for ra, rb, off, ov in _pairs(c):
        g = (torch.arange(ov, dtype=x.dtype) + 1) / (ov + 1)
        a, b = x[ra, :, off:off + ov].clone(), x[rb, :, :ov].clone()
        m = a + g * (b - a)
        x[ra, :, off:off + ov] = m
        x[rb, :, :ov] = m
    return x


def _i32(v):
    return (C.c_int32 * max(len(v), 1))(*v)


@pytest.fixture(scope="module")
def mixed(clips):
    return _call(clips)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_blend_unit(ctx, mixed):
    lib = ctx.lib
    c = mixed
    assert _pairs(c) == [(0, 2, 32, 8), (1, 4, 30, 10), (2, 7, 28, 12), (5, 8, 32, 8), (6, 9, 32, 8), (9, 10, 8, 8)]
    x0 = torch.randn(11, NCH, T, generator=torch.Generator().manual_seed(99))
    for r, m in enumerate(c["lens"]):
        x0[r, :, m:] = float("nan")                  # the padding behind each row's length: neither read nor written
    x = x0.cuda()
    args = (_i32(c["group"]), _i32(c["start"]), _i32(c["lens"]), 11, NCH, T, L.stream_ptr())
    assert lib.vb_window_rows_blend(L.ptr(x), *args) == 0, lib.vb_last_error()
    torch.cuda.synchronize()
    got = x.cpu()
    src = x0.numpy()
    want = src.astype(np.float64)
    touched = np.zeros(x0.shape, dtype=bool)
    for ra, rb, off, ov in _pairs(c):
        gw = ((np.arange(ov, dtype=np.float32) + np.float32(1)) / np.float32(ov + 1)).astype(np.float32)
        xa, xb = src[ra, :, off:off + ov], src[rb, :, :ov]
        d = (xb - xa).astype(np.float32)
        m = xa.astype(np.float64) + gw.astype(np.float64) * d.astype(np.float64)
        want[ra, :, off:off + ov] = m
        want[rb, :, :ov] = m
        assert not touched[ra, :, off:off + ov].any() and not touched[rb, :, :ov].any(), "the pairs are disjoint"
        touched[ra, :, off:off + ov] = True
        touched[rb, :, :ov] = True
    assert touched.sum() == 2 * NCH * (8 + 10 + 12 + 8 + 8 + 8)
    assert np.isfinite(got.numpy()[touched]).all(), "padding reached an overlap"
    err, mx = float(np.abs(got.numpy()[touched].astype(np.float64) - want[touched]).max()), float(np.abs(want[touched]).max())
    print(f"vb_window_rows_blend vs float64 restatement: max|diff| = {err:.3e} = {err / mx:.3e} of max-abs {mx:.4g} (bound {ALL_ONE:.0e})")
    assert err <= ALL_ONE * mx
    assert np.array_equal(got.numpy().view(np.int32)[~touched], src.view(np.int32)[~touched]), "an element outside the overlaps changed (NaN padding included)"
    assert not np.array_equal(got.numpy()[touched], src[touched])
    _assert_overlaps_agree(got, c, "after vb_window_rows_blend")
    again = got.clone().cuda()
    assert lib.vb_window_rows_blend(L.ptr(again), *args) == 0
    # len == NULL: every row has T tokens (the uniform plan of tests/test_gpu_joint.py equals vb_window_blend bit for bit)
    u0 = torch.randn(6, NCH, T, generator=torch.Generator().manual_seed(3))
    ua, ub = u0.cuda(), u0.cuda()
    assert lib.vb_window_rows_blend(L.ptr(ua), _i32([0, 1] * 3), _i32([0, 0, 32, 32, 60, 60]), None, 6, NCH, T, L.stream_ptr()) == 0
    assert lib.vb_window_blend(L.ptr(ub), _i32([0, 32, 60]), 3, 6, NCH, T, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.int32), got.numpy().view(np.int32)), "a second application changed something"
    assert torch.equal(ua, ub) and not torch.equal(ua.cpu(), u0)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("prec", ["split", "bf16"])
def test_the_uniform_plan_equals_vb_windows_bit_for_bit(engines, prec):
    """B = 2 clips of 100 tokens, starts (0, 32, 60), row = w * 2 + b (tests/test_gpu_joint.py), written as window rows"""
    eng = engines[prec]
    BC, STARTS = 2, (0, 32, 60)
    inp = clip_batch(BC, 100, LC)
    x = torch.cat([inp["x_latent"][:, :, s:s + T] for s in STARTS]).contiguous()
    midi = torch.cat([inp["midi"][..., 2 * s:2 * (s + T)] for s in STARTS]).contiguous()
    beats = torch.cat([inp["beats"][..., 2 * s:2 * (s + T)] for s in STARTS]).contiguous()
    t5 = torch.cat([inp["t5_cond"].repeat(3, 1, 1), inp["t5_uncond"].repeat(3, 1, 1)])
    idx, dts = vm.euler_tables(4)
    cond = eng.precompute_cond(t5, midi, beats, T)
    xa, ta = eng.sample_cfg(x, cond, idx, dts, 3.0, seed=5, clip_base=6, return_traj=True, windows=STARTS)
    xb, tb = eng.sample_cfg(x, cond, idx, dts, 3.0, seed=5, clip_base=6, return_traj=True,
                            window_rows=([r % BC for r in range(6)], [STARTS[r // BC] for r in range(6)]))
    _, tp = eng.sample_cfg(x, cond, idx, dts, 3.0, seed=5, clip_base=6, return_traj=True)
    torch.cuda.synchronize()
    assert torch.isfinite(ta).all() and not torch.equal(ta[1], tp[1]), "the consensus must do something"
    for k in range(4):
        assert torch.equal(ta[k], tb[k]), describe(f"{prec} traj[{k}]: window rows vs vb_windows", tb[k], ta[k])
    assert torch.equal(xa, xb)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def mixed_trajs(engines, mixed):
    """the 3-step trajectory of the mixed call per precision: computed once, shared, left unchanged"""
    idx, dts = vm.euler_tables(4)
    out = {}
    for prec in ("bf16", "split"):
        x, traj = _sample(engines[prec], mixed, idx, dts, return_traj=True)
        out[prec] = (x.cpu(), traj.cpu())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", ["bf16", "split"])
@pytest.mark.parametrize("g", list("ABCDE"))
def test_a_group_does_not_depend_on_the_other_groups(engines, clips, mixed, mixed_trajs, prec, g):
    """the rows of group g in the mixed call hold the bits of the same entry point on that group's rows alone, with the same noise keys;
    this is the test a wrong pair table fails"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    x, traj = mixed_trajs[prec]
    assert torch.isfinite(traj).all()
    for k in range(4):
        _assert_overlaps_agree(traj[k], mixed, f"{prec} mixed traj[{k}]")
    rows = [r for r, (h, _) in enumerate(ORDER) if h == g]
    alone = _call(clips, [ORDER[r] for r in rows])
    xa, ta = _sample(eng, alone, idx, dts, return_traj=True)
    torch.cuda.synchronize()
    xa, ta = xa.cpu(), ta.cpu()
    for i, r in enumerate(rows):
        m = mixed["lens"][r]
        for k in range(4):
            assert torch.equal(traj[k, r, :, :m], ta[k, i, :, :m]), describe(f"{prec} group {g} row {r} state {k}", traj[k, r, :, :m], ta[k, i, :, :m])
        assert torch.equal(x[r, :, :m], xa[i, :, :m]) and not x[r, :, m:].any()
    if g == "C":        # no pair: the plain call of a 25-token clip
        c = clips["C"]
        cond = eng.precompute_cond(torch.stack([c["t5_cond"], c["t5_uncond"]]), c["midi"], c["beats"], 25)
        _, tp = eng.sample_cfg(c["x_latent"][None], cond, idx, dts, 3.0, seed=5, clip_ids=[_key("C", 0)], return_traj=True)
        torch.cuda.synchronize()
        assert torch.equal(tp.cpu()[:, 0], traj[:, rows[0], :, :25]), "group C vs the plain call of the clip alone"


# ---------------------------------------------------------------------------------------------------------------- 4
def test_group_d_follows_the_cpu_restatement(engines, sd, clips):
    """split precision, injected router noise, 3 steps, group D as 2 rows (40 and 17 tokens) at T = 40: every state against
    ref_cpu.dit_forward on each row's own tokens + CFG + Euler + the consensus written in torch, equal routing at every state"""
    eng = engines["split"]
    cfg = synth.DiTConfig()
    c = _call(clips, [("D", 0), ("D", 1)])
    lens, B, timesteps, scale = c["lens"], 2, 4, 3.0
    idx, dts = vm.euler_tables(timesteps)
    steps, E, depth = len(idx), cfg.num_experts, cfg.depth
    noise_steps = [[exp_noise(B, T, E, 2 * k + br, depth) for br in (0, 1)] for k in range(steps)]
    cond = eng.precompute_cond(c["t5"], c["midi"], c["beats"], T, lengths=lens)
    x, traj = eng.sample_cfg(c["x"], cond, idx, dts, scale, noise=gumbel_arrays_steps(noise_steps), return_traj=True,
                             window_rows=(c["group"], c["start"]), lengths=lens)
    torch.cuda.synchronize()
    traj = traj.cpu()
    assert torch.equal(x.cpu(), traj[-1]) and torch.isfinite(traj).all()
    for k in range(steps + 1):
        _assert_overlaps_agree(traj[k], c, f"traj[{k}]")

    def row_noise(nz, b):
        return [tuple(e[b * T:b * T + lens[b]] for e in blk) for blk in nz]

    pre = [[ref_cpu.dit_precompute(sd, t5[b:b + 1], c["midi"][b:b + 1, None, :2 * lens[b]], c["beats"][b:b + 1, None, :2 * lens[b]], lens[b]) for b in range(B)]
           for t5 in (c["tc"], c["tu"])]
    t_span, tidx = ref_cpu.t_index_table(timesteps, None)
    xr = _blend_torch(c["x"], c)
    want, routes = [xr.clone()], []
    t = t_span[0]
    for k in range(steps):
        dt = t_span[k + 1] - t
        ti = torch.full((1,), tidx[k], dtype=torch.long)
        xn, aux = xr.clone(), []
        for b in range(B):
            xb = xr[b:b + 1, :, :lens[b]]
            e_c, aux_c = ref_cpu.dit_forward(sd, xb, ti, pre[0][b], row_noise(noise_steps[k][0], b), return_aux=True)
            e_u, aux_u = ref_cpu.dit_forward(sd, xb, ti, pre[1][b], row_noise(noise_steps[k][1], b), return_aux=True)
            xn[b:b + 1, :, :lens[b]] = xb + dt * (e_u + scale * (e_c - e_u))
            aux.append((aux_c, aux_u))
        xr = _blend_torch(xn, c)
        t = t + dt
        want.append(xr.clone())
        routes.append(aux)
    for k in range(steps + 1):
        for b in range(B):
            got, ref = traj[k][b, :, :lens[b]], want[k][b, :, :lens[b]]
            err = rel_l2(got, ref)
            print(f"group D, state {k}, row {b}: rel_l2 = {err:.3e} (bound 1e-3)")
            assert err < 1e-3, describe(f"state {k} row {b} vs restatement", got, ref)
    N = B * T
    for k in range(steps):
        t_idx = torch.full((2 * B,), idx[k], dtype=torch.int64)
        _, got = eng.forward(traj[k], t_idx, cond, noise=gumbel_arrays(noise_steps[k]), return_routes=True, lengths=lens)
        torch.cuda.synchronize()
        for br in (0, 1):
            for i in range(depth):
                for j, name in ((0, "ic"), (1, "ia")):
                    for b in range(B):
                        r_got = got[i, j, br * N + b * T:br * N + b * T + lens[b]].cpu().long()
                        r_ref = routes[k][b][br][f"{name}{i}"]
                        assert torch.equal(r_got, r_ref), f"step {k} branch {br} block {i} {name} row {b}: {int((r_got != r_ref).sum())} tokens route differently"


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_padding_is_never_read(engines, clips, mixed, mixed_trajs, prec):
    """the mixed call again with other finite garbage in the padding of x, midi and beats: bit-identical on valid tokens"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    other = _call(clips, pad_x=-7.5e3, pad_track=57)
    assert not torch.equal(other["x"], mixed["x"]) and not torch.equal(other["midi"], mixed["midi"]) and not torch.equal(other["beats"], mixed["beats"])
    _, second = _sample(eng, other, idx, dts, return_traj=True)
    torch.cuda.synchronize()
    second, first = second.cpu(), mixed_trajs[prec][1]
    for r, m in enumerate(mixed["lens"]):
        assert torch.equal(first[:, r, :, :m], second[:, r, :, :m]), describe(f"{prec} row {r}: other padding, other result", second[:, r, :, :m], first[:, r, :, :m])


# ---------------------------------------------------------------------------------------------------------------- 6
def _path(t, ref, x0, sigma=SIGMA):
    """r(t) on the host in float32"""
    t = np.float32(t)
    c0 = np.float32(1) - np.float32(np.float32(1) - np.float32(sigma)) * t
    return torch.from_numpy((t * ref.numpy().astype(np.float32) + np.float32(c0) * x0.numpy().astype(np.float32)).astype(np.float32))


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_fused_update_equals_the_separate_launches_bit_for_bit(engines, mixed, mixed_trajs, knobs, prec):
    """the consensus is one kernel behind either update form: VB_EULER_LAUNCH=1 must not move a bit - plain, with a known region that is
    equal in both copies of an overlap (clip A's tokens 30..38: row 0's 30..38 and row 2's 0..6, ref and x0 cut from the long clip), and
    under a guidance schedule with a weight-0 step"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    times = vm.euler_times(4)
    mask = torch.zeros(11, T)
    mask[0, 30:38] = 1.0
    mask[2, 0:6] = 1.0
    keep = (mixed["ref"], mixed["x"], mask, times, SIGMA)
    sched = [1.0, 0.0, 0.5]
    outs = {}
    for knob in ("fused", "VB_EULER_LAUNCH"):
        knobs(**({knob: "1"} if knob != "fused" else {}))
        outs[knob] = [_sample(eng, mixed, idx, dts, return_traj=True)[1].cpu(), _sample(eng, mixed, idx, dts, return_traj=True, keep=keep)[1].cpu(),
                      _sample(eng, mixed, idx, dts, return_traj=True, guidance=sched)[1].cpu(),
                      _sample(eng, mixed, idx, dts, return_traj=True, keep=keep, guidance=sched)[1].cpu()]
        torch.cuda.synchronize()
    a, b = outs["fused"], outs["VB_EULER_LAUNCH"]
    assert torch.equal(a[0], mixed_trajs[prec][1])
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[0], a[2]) and not torch.equal(a[1], a[3])
    for i, what in enumerate(("plain", "keep", "schedule", "keep + schedule")):
        assert torch.isfinite(a[i]).all()
        assert torch.equal(a[i], b[i]), describe(f"{prec} window rows, {what}: fused vs separate launches", b[i], a[i])
        for k in range(4):
            _assert_overlaps_agree(b[i][k], mixed, f"{prec} {what} traj[{k}]")
    for i in (1, 3):
        for k in range(len(idx)):
            for r, sl in ((0, slice(30, 38)), (2, slice(0, 6))):
                got, want = a[i][k + 1][r, :, sl], _path(times[k], mixed["ref"], mixed["x"])[r, :, sl]
                err, mx = float((got - want).abs().max()), float(want.abs().max())
                print(f"{prec}: kept tokens of row {r} after step {k}: max|diff| = {err:.3e} = {err / mx:.3e} of max-abs (bound {ALL_ONE:.0e})")
                assert err <= ALL_ONE * mx


# ---------------------------------------------------------------------------------------------------------------- 7
def test_graph_replay_equals_eager_and_keys_on_the_plan(ctx, sd, engines, clips, mixed, mixed_trajs, knobs):
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(4)
    dev = {k: mixed[k].cuda() for k in ("x", "midi", "beats", "t5")}
    # another plan on the same buffers: group E's last row starts one token later (its overlap with the middle row shrinks to 7)
    other_start = list(mixed["start"])
    other_start[10] = 41
    stream = torch.cuda.Stream()
    kw = dict(seed=5, clip_ids=mixed["keys"], lengths=mixed["lens"])
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(dev["t5"], dev["midi"], dev["beats"], T, persistent=True, lengths=mixed["lens"])
        a = [eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, window_rows=(mixed["group"], mixed["start"]), **kw).cpu() for _ in range(3)]
        stream.synchronize()
        assert eng.graphs() == 1, "the repeated window-rows call was not captured"
        b = [eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, window_rows=(mixed["group"], other_start), **kw).cpu() for _ in range(3)]
        stream.synchronize()
        assert eng.graphs() == 2, "another plan on the same buffers must capture its own graph"
        a.append(eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, window_rows=(list(mixed["group"]), list(mixed["start"])), **kw).cpu())   # by value
        lens_only = [eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, **kw).cpu() for _ in range(3)]
        stream.synchronize()
        assert eng.graphs() == 3, "a lengths-only call never replays a window-rows graph"
        # no group with two rows: the lengths-only call, and its graph
        solo = eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, window_rows=(list(range(11)), mixed["start"]), **kw).cpu()
        stream.synchronize()
        assert eng.graphs() == 3 and torch.equal(solo, lens_only[0])
    want = mixed_trajs["bf16"][0]
    for rep in range(4):
        assert torch.equal(a[rep], want), describe(f"window rows, call {rep} vs the eager call", a[rep], want)
    assert torch.equal(b[0], b[1]) and torch.equal(b[0], b[2]) and not torch.equal(b[0], a[0])
    others = [r for r, (g, _) in enumerate(ORDER) if g != "E"]
    assert torch.equal(b[0][others], a[0][others]), "the other plan moves group E's rows alone"
    assert torch.equal(lens_only[0], lens_only[2]) and not torch.equal(lens_only[0], a[0])
    # a plain call and a windows= call afterwards are what they are on an engine that never saw window rows
    inp = clip_batch(2, 100, LC)
    STARTS = (0, 32, 60)
    x = torch.cat([inp["x_latent"][:, :, s:s + T] for s in STARTS]).contiguous().cuda()
    midi = torch.cat([inp["midi"][..., 2 * s:2 * (s + T)] for s in STARTS]).contiguous().cuda()
    beats = torch.cat([inp["beats"][..., 2 * s:2 * (s + T)] for s in STARTS]).contiguous().cuda()
    t5 = torch.cat([inp["t5_cond"].repeat(3, 1, 1), inp["t5_uncond"].repeat(3, 1, 1)]).cuda()
    res = {}
    for name, e in (("seen", eng), ("fresh", _fresh(ctx, sd, engines))):
        with torch.cuda.stream(stream):
            cond = e.precompute_cond(t5, midi, beats, T, persistent=True)
            res[name] = [e.sample_cfg(x, cond, idx, dts, 3.0, seed=7).cpu() for _ in range(3)] + \
                        [e.sample_cfg(x, cond, idx, dts, 3.0, seed=7, windows=STARTS).cpu() for _ in range(3)]
            stream.synchronize()
    for i in range(6):
        assert torch.equal(res["seen"][i], res["fresh"][i]), f"call {i} after window-rows calls vs a fresh engine"
    assert not torch.equal(res["seen"][0], res["seen"][3])


# ---------------------------------------------------------------------------------------------------------------- 8
def test_refusals_name_the_row_and_leave_x_unchanged(engines, mixed):
    eng = engines["bf16"]
    lib = eng.ctx.lib
    idx, dts = vm.euler_tables(4)
    cond = eng.precompute_cond(mixed["t5"], mixed["midi"], mixed["beats"], T, lengths=mixed["lens"])
    x = mixed["x"].cuda()
    before = x.clone()
    tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
    ws = eng._workspace(11, 2, T, LC)
    ns = L.Noise()

    def sample(group, start, lens=mixed["lens"], win=None, B=11):
        wr = L.WindowRows(_i32(group) if group is not None else None, _i32(start) if start is not None else None)
        ls = L.Lens(_i32(lens)) if lens is not None else None
        rc = lib.vb_sample_cfg_window_rows(eng.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, 2, T, LC, 3, L.ptr(tt), L.ptr(dd), 3.0, C.byref(wr),
                                           C.byref(ls) if ls is not None else None, None, C.byref(win) if win is not None else None, None, None,
                                           C.byref(ns), None, L.ptr(ws), L.stream_ptr())
        return rc, lib.vb_last_error()

    G, S = mixed["group"], mixed["start"]

    def put(v, r, val):
        v = list(v)
        v[r] = val
        return v

    cases = [((None, S), b"group"), ((G, None), b"start"),
             ((G, put(S, 3, -1)), b"row 3"),                      # start < 0
             ((G, put(S, 7, 20)), b"row 7"),                      # A2 before A1: not ascending
             ((G, put(S, 7, 32)), b"row 7"),                      # start[rb] <= start[ra]
             ((G, put(S, 4, 41)), b"row 4"),                      # B1 leaves a gap behind B0
             ((G, put(S, 8, 20)), b"row 8"),                      # D1 (17 tokens) inside its overlap of 20
             ((G, put(S, 10, 39)), b"row 10"),                    # E2 reaches into E0: a token under three rows
             ((G, put(S, 7, 39)), b"row 7")]                      # A2 reaches into A0
    for (group, start), needle in cases:
        rc, msg = sample(group, start)
        assert rc == VB_E_INVALID and needle in msg, (start, msg)
    rc, msg = sample([0] * 65, list(range(65)), lens=None, B=65)
    assert rc == VB_E_INVALID and b"row 64" in msg, msg
    rc, msg = sample([0] * 65, list(range(65)), lens=[T] * 65, B=65)
    assert rc == VB_E_INVALID and b"row 64" in msg, msg
    starts = _i32([0, 32])
    rc, msg = sample([r % 2 for r in range(10)], [0] * 10, lens=None, win=L.Windows(starts, 2), B=10)
    assert rc == VB_E_INVALID and b"window" in msg and b"row 0" in msg, msg
    # the refusal of win beside lengths stays, word for word
    rc, msg = sample(G, S, win=L.Windows(starts, 2), B=10)
    assert rc == VB_E_INVALID and b"row 3 has length 25 of 40 beside 2 joint windows, which are equal-length by construction" in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(x, before), "a refused call must not touch x"
    with pytest.raises(ValueError, match="row 10 at 39 reaches into row 6"):
        eng.sample_cfg(mixed["x"], cond, idx, dts, 3.0, window_rows=(G, put(S, 10, 39)), lengths=mixed["lens"])


# ---------------------------------------------------------------------------------------------------------------- 9
def test_sample_long_with_lengths_equals_every_clip_alone(ctx, sd, engines, clips):
    """sample_long(lengths=[100, 70, 25], mode="joint", window=40, overlap=8): clip b is sample_long on that clip alone with clip_base + b,
    bit for bit; zeros behind each clip's end; every window's bits are what the stitch holds"""
    eng = _fresh(ctx, sd, engines)
    lengths, Tmax, base = [100, 70, 25], 100, 4
    idx, dts = vm.euler_tables(4)
    x0 = _rnd((3, NCH, Tmax), "long_pad", 0.5)
    midi, beats = torch.full((3, 1, 2 * Tmax), 57, dtype=torch.int64), torch.full((3, 1, 2 * Tmax), 1, dtype=torch.int64)
    for b, g in enumerate("ABC"):
        n = lengths[b]
        x0[b, :, :n] = clips[g]["x_latent"]
        midi[b, 0, :2 * n] = clips[g]["midi"][0]
        beats[b, 0, :2 * n] = clips[g]["beats"][0]
    tc, tu = torch.stack([clips[g]["t5_cond"] for g in "ABC"]), torch.stack([clips[g]["t5_uncond"] for g in "ABC"])
    kw = dict(window=40, overlap=8, seed=3, mode="joint")
    z, parts = longform.sample_long(eng, x0, tc, tu, midi, beats, idx, dts, 3.0, clip_base=base, lengths=lengths, return_windows=True, **kw)
    torch.cuda.synchronize()
    assert z.shape == (3, NCH, Tmax) and torch.isfinite(z).all()
    for b, n in enumerate(lengths):
        alone = longform.sample_long(eng, x0[b:b + 1, :, :n].contiguous(), tc[b:b + 1], tu[b:b + 1], midi[b:b + 1, :, :2 * n].contiguous(),
                                     beats[b:b + 1, :, :2 * n].contiguous(), idx, dts, 3.0, clip_base=base + b, **kw)
        torch.cuda.synchronize()
        assert torch.equal(z[b:b + 1, :, :n], alone), describe(f"clip {b} ({n} tokens) in the mixed call vs alone", z[b:b + 1, :, :n], alone)
        assert not z[b, :, n:].any(), "zeros behind the clip's end"
        plan = longform.plan_windows(n, 40, 8)
        assert len(parts[b]) == len(plan)
        for (s, m), p in zip(plan, parts[b]):
            assert torch.equal(z[b:b + 1, :, s:s + m], p), f"clip {b}: the window at {s} is not what the stitch holds"
    with pytest.raises(ValueError, match='lengths belong to mode="joint"'):
        longform.sample_long(eng, x0, tc, tu, midi, beats, idx, dts, 3.0, window=40, overlap=8, lengths=lengths)
