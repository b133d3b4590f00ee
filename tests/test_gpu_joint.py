"""Joint window sampling on the GPU (vb_sample_cfg_windows, vb_window_blend, through the C ABI): all windows of a long clip ride as rows of
one sampler call, and after every Euler step the overlapping tokens of neighbouring windows take one consensus value
m = fmaf(g, x[ib] - x[ia], x[ia]), g = (u + 1) / (ov + 1).

The small plan is B = 2 clips, T = 100, window 40, overlap 8: starts (0, 32, 60), overlaps 8 and 12 - three windows, a shifted last window
with another overlap, two clips interleaved in the row index (row = w * 2 + b).

Bounds.  The blend unit is compared with a float64 restatement that forms d = float32(xb - xa) and g = float32(u + 1) / float32(ov + 1) in
fp32 first: the device does one fma rounding, the restatement a float64 rounding and then an fp32 rounding - together at most 1 ulp of
|m| <= max-abs, 2e-7 of max-abs.  The trajectory is compared with a CPU restatement over oracle.ref_cpu.dit_forward at the project's 3-step
CFG-trajectory bound, rel-L2 1e-3 (tests/test_gpu_path.py; the blend is a convex combination and does not widen it), with equal routing
indices.  A kept token is compared with the host's r(t) at 2e-7 of max-abs, as tests/test_gpu_keep.py does.  Everything that claims "the same
arithmetic" or "the same bits" is compared bit for bit."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, clip_batch, describe, exp_noise, gumbel_arrays, gumbel_arrays_steps, rel_l2
from versband_amd import _lib as L
from versband_amd import longform
from versband_amd import model as vm
from versband_amd import synth

pytestmark = pytest.mark.gpu
SIGMA = 1e-4            # CFM.sigma_min (versband_amd/model.py)
ALL_ONE = 2e-7          # of the tensor's max-abs
BC, T_LONG, WIN, OVL, LC = 2, 100, 40, 8, 8
STARTS = (0, 32, 60)
NW = len(STARTS)
VB_E_INVALID = -1


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


def _rows(inp, starts=STARTS, n=WIN, clips=slice(None)):
    """the rows sample_long builds for the plan: x / midi / beats slices and the repeated captions, row = w * Bc + b"""
    x = torch.cat([inp["x_latent"][clips, :, s:s + n] for s in starts]).contiguous()
    midi = torch.cat([inp["midi"][clips][..., 2 * s:2 * (s + n)] for s in starts]).contiguous()
    beats = torch.cat([inp["beats"][clips][..., 2 * s:2 * (s + n)] for s in starts]).contiguous()
    nw = len(starts)
    tc, tu = inp["t5_cond"][clips].repeat(nw, 1, 1), inp["t5_uncond"][clips].repeat(nw, 1, 1)
    return x, midi, beats, tc, tu


@pytest.fixture(scope="module")
def small():
    inp = clip_batch(BC, T_LONG, LC)
    x, midi, beats, tc, tu = _rows(inp)
    return dict(inp=inp, x=x, midi=midi, beats=beats, tc=tc, tu=tu, t5=torch.cat([tc, tu]))


def _overlaps(starts, n):
    return [starts[w] + n - starts[w + 1] for w in range(len(starts) - 1)]


def _assert_overlaps_agree(x, starts, Bc, what):
    """token n - ov + u of row w*Bc + b and token u of row (w+1)*Bc + b hold the same bits"""
    n = x.shape[-1]
    for w, ov in enumerate(_overlaps(starts, n)):
        a, b = x[w * Bc:(w + 1) * Bc, :, n - ov:], x[(w + 1) * Bc:(w + 2) * Bc, :, :ov]
        assert torch.equal(a, b), describe(f"{what}: overlap of windows {w} / {w + 1} ({ov} tokens)", a, b)


def _blend_torch(x, starts, Bc):
    """the consensus written in torch, in x's dtype"""
    x = x.clone()
    n = x.shape[-1]
    for w, ov in enumerate(_overlaps(starts, n)):
        if ov <= 0:
            continue
        g = (torch.arange(ov, dtype=x.dtype) + 1) / (ov + 1)
        a, b = x[w * Bc:(w + 1) * Bc, :, n - ov:].clone(), x[(w + 1) * Bc:(w + 2) * Bc, :, :ov].clone()
        m = a + g * (b - a)
        x[w * Bc:(w + 1) * Bc, :, n - ov:] = m
        x[(w + 1) * Bc:(w + 2) * Bc, :, :ov] = m
    return x


def _blend_call(lib, x, starts, B=None, n=None):
    arr = (C.c_int32 * max(len(starts), 1))(*starts)
    return lib.vb_window_blend(L.ptr(x), arr, len(starts), x.shape[0] if B is None else B, x.shape[1], x.shape[2] if n is None else n, L.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------- 1
def test_the_blend_unit(ctx):
    lib = ctx.lib
    g = torch.Generator().manual_seed(99)
    x0 = torch.randn(NW * BC, 20, WIN, generator=g)
    x = x0.cuda()
    assert _blend_call(lib, x, STARTS) == 0
    torch.cuda.synchronize()
    got = x.cpu()
    # float64 restatement over the fp32 difference and the fp32 weight
    want = x0.numpy().astype(np.float64)
    touched = np.zeros(x0.shape, dtype=bool)
    src = x0.numpy()
    for w, ov in enumerate(_overlaps(STARTS, WIN)):
        gw = ((np.arange(ov, dtype=np.float32) + np.float32(1)) / np.float32(ov + 1)).astype(np.float32)
        ra, rb = slice(w * BC, (w + 1) * BC), slice((w + 1) * BC, (w + 2) * BC)
        xa, xb = src[ra, :, WIN - ov:], src[rb, :, :ov]
        d = (xb - xa).astype(np.float32)
        m = xa.astype(np.float64) + gw.astype(np.float64) * d.astype(np.float64)
        want[ra, :, WIN - ov:] = m
        want[rb, :, :ov] = m
        touched[ra, :, WIN - ov:] = True
        touched[rb, :, :ov] = True
    err, mx = float(np.abs(got.numpy().astype(np.float64) - want).max()), float(np.abs(want).max())
    print(f"vb_window_blend vs float64 restatement: max|diff| = {err:.3e} = {err / mx:.3e} of max-abs {mx:.4g} (bound {ALL_ONE:.0e})")
    assert err <= ALL_ONE * mx
    assert touched.sum() == 2 * BC * 20 * (8 + 12)
    assert np.array_equal(got.numpy()[~touched], src[~touched]), "an element outside the overlaps changed"
    assert not np.array_equal(got.numpy()[touched], src[touched])
    _assert_overlaps_agree(got, STARTS, BC, "after vb_window_blend")
    # rows that agree already come back bit for bit: a second pass, and rows cut from one long tensor
    again = got.clone().cuda()
    assert _blend_call(lib, again, STARTS) == 0
    long = torch.randn(BC, 20, T_LONG, generator=g)
    cut = torch.cat([long[:, :, s:s + WIN] for s in STARTS]).contiguous()
    cut_d = cut.cuda()
    assert _blend_call(lib, cut_d, STARTS) == 0
    # touching windows (no overlap) and one window: nothing to do
    same = x0.cuda()
    assert _blend_call(lib, same, (0, 40, 80)) == 0 and _blend_call(lib, same, (7,)) == 0
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), got) and torch.equal(cut_d.cpu(), cut) and torch.equal(same.cpu(), x0)
    # malformed plans: the error code, nothing launched
    keep = x0.cuda()
    for starts, B in (((0, 32, 73), 6), ((0, 41), 6), ((32, 0), 6), ((0, 40, 40), 6), ((0, 32, 39), 6), ((0, 10, 20), 6), ((-1, 32, 60), 6),
                      ((0, 32, 60), 4), ((0, 30, 60, 90), 6), ((), 6), (tuple(range(0, 65 * 40, 40)), 65)):
        assert _blend_call(lib, keep, starts, B=B) == VB_E_INVALID, starts
        assert lib.vb_last_error()
    assert lib.vb_window_blend(L.ptr(keep), None, 3, 6, 20, WIN, L.stream_ptr()) == VB_E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(keep.cpu(), x0)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_trajectory_follows_the_cpu_restatement(engines, sd, small):
    """split precision, injected router noise, 3 steps, the small plan as 6 rows of 40 tokens: every state against ref_cpu.dit_forward per
    branch + CFG + Euler + the blend written in torch, equal routing at every state, equal bits in every overlap of every state"""
    eng = engines["split"]
    cfg = synth.DiTConfig()
    B, n, timesteps, scale = NW * BC, WIN, 4, 3.0
    idx, dts = vm.euler_tables(timesteps)
    steps = len(idx)
    E, depth = cfg.num_experts, cfg.depth
    noise_steps = [[exp_noise(B, n, E, 2 * k + br, depth) for br in (0, 1)] for k in range(steps)]
    cond = eng.precompute_cond(small["t5"], small["midi"], small["beats"], n)
    x, traj = eng.sample_cfg(small["x"], cond, idx, dts, scale, noise=gumbel_arrays_steps(noise_steps), return_traj=True, windows=STARTS)
    torch.cuda.synchronize()
    traj = traj.cpu()
    assert torch.equal(x.cpu(), traj[-1]) and torch.isfinite(traj).all()
    assert torch.equal(traj[0], small["x"]), "rows cut from one start noise: the entry consensus changes nothing"
    for k in range(steps + 1):
        _assert_overlaps_agree(traj[k], STARTS, BC, f"traj[{k}]")
    # the restatement
    cc = ref_cpu.dit_precompute(sd, small["tc"], small["midi"], small["beats"], n)
    cu = ref_cpu.dit_precompute(sd, small["tu"], small["midi"], small["beats"], n)
    t_span, tidx = ref_cpu.t_index_table(timesteps, None)
    xr = _blend_torch(small["x"], STARTS, BC)
    want, routes = [xr.clone()], []
    t = t_span[0]
    for k in range(steps):
        dt = t_span[k + 1] - t
        ti = torch.full((B,), tidx[k], dtype=torch.long)
        e_c, aux_c = ref_cpu.dit_forward(sd, xr, ti, cc, noise_steps[k][0], return_aux=True)
        e_u, aux_u = ref_cpu.dit_forward(sd, xr, ti, cu, noise_steps[k][1], return_aux=True)
        xr = _blend_torch(xr + dt * (e_u + scale * (e_c - e_u)), STARTS, BC)
        t = t + dt
        want.append(xr.clone())
        routes.append((aux_c, aux_u))
    want = torch.stack(want)
    for k in range(steps + 1):
        err = rel_l2(traj[k], want[k])
        print(f"joint windows, state {k}: rel_l2 = {err:.3e} (bound 1e-3)")
        assert err < 1e-3, describe(f"state {k} vs restatement", traj[k], want[k])
    # the blend did something: without it the windows drift apart in their overlaps
    _, plain = eng.sample_cfg(small["x"], cond, idx, dts, scale, noise=gumbel_arrays_steps(noise_steps), return_traj=True)
    torch.cuda.synchronize()
    assert torch.equal(plain[1].cpu(), traj[1]) is False
    assert not torch.equal(plain[-1].cpu()[:BC, :, n - 8:], plain[-1].cpu()[BC:2 * BC, :, :8])
    # routing: the network evaluated at each state of the GPU trajectory routes like the oracle did at its own
    N = B * n
    for k in range(steps):
        t_idx = torch.full((2 * B,), idx[k], dtype=torch.int64)
        _, got = eng.forward(traj[k], t_idx, cond, noise=gumbel_arrays(noise_steps[k]), return_routes=True)
        torch.cuda.synchronize()
        for br in (0, 1):
            for i in range(depth):
                for j, name in ((0, "ic"), (1, "ia")):
                    r_got = got[i, j, br * N:(br + 1) * N].cpu().long()
                    assert torch.equal(r_got, routes[k][br][f"{name}{i}"]), \
                        f"step {k} branch {br} block {i} {name}: {int((r_got != routes[k][br][f'{name}{i}']).sum())} tokens route differently"


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_fused_update_equals_the_separate_launches_bit_for_bit(engines, small, monkeypatch, prec):
    """the consensus is one kernel behind either update form: VB_EULER_LAUNCH=1 must not move a bit, with and without a known region"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    B = NW * BC
    mask = torch.zeros(B, WIN)
    mask[:BC, :12] = 1.0
    keep = (torch.randn(small["x"].shape, generator=torch.Generator().manual_seed(5)), small["x"], mask, vm.euler_times(4), SIGMA)
    outs = []
    try:
        for knob in (None, "VB_EULER_LAUNCH"):
            if knob:
                monkeypatch.setenv(knob, "1")
            L.load().vb_tune_reload()
            cond = eng.precompute_cond(small["t5"], small["midi"], small["beats"], WIN)
            a = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=21, windows=STARTS)
            b = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=21, windows=STARTS, keep=keep)
            torch.cuda.synchronize()
            outs.append((a.clone(), b.clone()))
            if knob:
                monkeypatch.delenv(knob)
    finally:
        monkeypatch.delenv("VB_EULER_LAUNCH", raising=False)
        L.load().vb_tune_reload()
    assert torch.isfinite(outs[0][0]).all() and not torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0][0], outs[1][0]), describe("joint: fused vs separate launches", outs[1][0], outs[0][0])
    assert torch.equal(outs[0][1], outs[1][1]), describe("joint + keep: fused vs separate launches", outs[1][1], outs[0][1])
    _assert_overlaps_agree(outs[1][0].cpu(), STARTS, BC, "separate launches")


def test_graph_replay_equals_eager_and_keys_on_the_plan(ctx, sd, engines, small, monkeypatch):
    """the captured loop holds the plan's values in its kernel arguments, so they are part of the graph key: another plan on the same buffers
    captures its own graph and gives its own result, and a plain call next to them is what it is on an engine that never saw a plan"""
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(6)
    t5, midi, beats, x0 = small["t5"].cuda(), small["midi"].cuda(), small["beats"].cuda(), small["x"].cuda()
    other = (0, 30, 60)                 # on rows cut at STARTS: the rows disagree in these overlaps on entry
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(t5, midi, beats, WIN, persistent=True)
        for rep in range(3):                         # eager, capture + replay, replay
            out[("a", rep)] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep, windows=STARTS)
        stream.synchronize()
        assert eng.graphs() == 1, "the repeated joint call was not captured"
        for rep in range(3):
            out[("b", rep)] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep, windows=other)
        stream.synchronize()
        assert eng.graphs() == 2, "another plan must capture its own graph"
        out[("a", 3)] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7, windows=list(STARTS))      # back to the first graph, by value
        for rep in range(3):
            out[("p", rep)] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep)
        stream.synchronize()
        assert eng.graphs() == 3
        for rep in range(2):                         # one window is the plain call: the plain graph replays, nothing new is captured
            out[("one", rep)] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep, windows=[5])
        stream.synchronize()
        assert eng.graphs() == 3
    assert torch.equal(out[("a", 0)], out[("a", 3)])
    assert not torch.equal(out[("a", 0)], out[("b", 0)]) and not torch.equal(out[("a", 0)], out[("p", 0)])
    assert torch.equal(out[("one", 0)], out[("p", 0)]) and torch.equal(out[("one", 1)], out[("p", 1)])
    for rep in range(3):
        _assert_overlaps_agree(out[("a", rep)].cpu(), STARTS, BC, f"plan a, call {rep}")
        _assert_overlaps_agree(out[("b", rep)].cpu(), other, BC, f"plan b, call {rep}")
    monkeypatch.setenv("VB_NO_GRAPH", "1")
    L.load().vb_tune_reload()
    try:
        eager = _fresh(ctx, sd, engines)             # never sees a plan before its plain calls
        with torch.cuda.stream(stream):
            cond = eager.precompute_cond(t5, midi, beats, WIN, persistent=True)
            for rep in range(3):
                want = eager.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep)
                stream.synchronize()
                assert torch.equal(want, out[("p", rep)]), describe(f"plain after joint calls vs a fresh engine, call {rep}", out[("p", rep)], want)
            for name, plan in (("a", STARTS), ("b", other)):
                for rep in range(3):
                    want = eager.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep, windows=plan)
                    stream.synchronize()
                    assert torch.equal(want, out[(name, rep)]), describe(f"graph vs eager, plan {name} call {rep}", out[(name, rep)], want)
        assert eager.graphs() == 0
    finally:
        monkeypatch.delenv("VB_NO_GRAPH", raising=False)
        L.load().vb_tune_reload()


def _path(t, ref, x0, sigma=SIGMA):
    """r(t) on the host in float32"""
    t = np.float32(t)
    c0 = np.float32(1) - np.float32(np.float32(1) - np.float32(sigma)) * t
    return torch.from_numpy((t * ref.cpu().numpy().astype(np.float32) + np.float32(c0) * x0.cpu().numpy().astype(np.float32)).astype(np.float32))


@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_joint_with_a_known_region(engines, small, prec):
    """an all-zero mask is joint sampling without keep, bit for bit; with the first 12 tokens of window 0 kept, those tokens sit on the path
    at every step and the overlaps still agree"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    times = vm.euler_times(4)
    B = NW * BC
    ref = torch.randn(small["x"].shape, generator=torch.Generator().manual_seed(6))
    cond = eng.precompute_cond(small["t5"], small["midi"], small["beats"], WIN)
    base = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=9, clip_base=4, windows=STARTS)
    zero = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=9, clip_base=4, windows=STARTS,
                          keep=(ref, small["x"], torch.zeros(B, WIN), times, SIGMA))
    mask = torch.zeros(B, WIN)
    mask[:BC, :12] = 1.0
    kept, traj = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=9, clip_base=4, windows=STARTS, keep=(ref, small["x"], mask, times, SIGMA),
                                return_traj=True)
    torch.cuda.synchronize()
    assert torch.isfinite(base).all() and torch.equal(base, zero), describe("zero mask vs joint without keep", zero, base)
    assert not torch.equal(kept, base)
    traj = traj.cpu()
    for k in range(len(idx)):
        got, want = traj[k + 1][:BC, :, :12], _path(times[k], ref, small["x"])[:BC, :, :12]
        err, mx = float((got - want).abs().max()), float(want.abs().max())
        print(f"{prec}: kept tokens after step {k}: max|diff| = {err:.3e} = {err / mx:.3e} of max-abs (bound {ALL_ONE:.0e})")
        assert err <= ALL_ONE * mx
        _assert_overlaps_agree(traj[k + 1], STARTS, BC, f"joint + keep, traj[{k + 1}]")


def test_a_clip_does_not_depend_on_its_neighbour_in_the_batch(engines, small):
    """clip b of Bc = 2 (rows b, 2 + b, 4 + b; noise keys clip_base + row) equals the same clip sampled alone as three rows with those keys"""
    eng = engines["bf16"]
    idx, dts = vm.euler_tables(4)
    base = 2 * NW
    cond = eng.precompute_cond(small["t5"], small["midi"], small["beats"], WIN)
    both = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=5, clip_base=base, windows=STARTS)
    torch.cuda.synchronize()
    for b in range(BC):
        x, midi, beats, tc, tu = _rows(small["inp"], clips=slice(b, b + 1))
        cond1 = eng.precompute_cond(torch.cat([tc, tu]), midi, beats, WIN)
        alone = eng.sample_cfg(x, cond1, idx, dts, 3.0, seed=5, clip_ids=[base + w * BC + b for w in range(NW)], windows=STARTS)
        torch.cuda.synchronize()
        assert torch.equal(alone, both[b::BC]), describe(f"clip {b} alone vs beside its neighbour", alone, both[b::BC])
        _assert_overlaps_agree(alone.cpu(), STARTS, 1, f"clip {b} alone")


def test_one_window_is_the_plain_call(engines, small):
    eng = engines["split"]
    idx, dts = vm.euler_tables(4)
    cond = eng.precompute_cond(small["t5"], small["midi"], small["beats"], WIN)
    _, plain = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=2, return_traj=True)
    _, one = eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=2, return_traj=True, windows=[0])
    torch.cuda.synchronize()
    assert torch.equal(plain, one)
    with pytest.raises(ValueError, match="three windows"):
        eng.sample_cfg(small["x"], cond, idx, dts, 3.0, seed=2, windows=[0, 10, 20])


# ---------------------------------------------------------------------------------------------------------------- 4
def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("B,T,window,overlap", [(2, 100, 40, 8), (1, 4500, 1500, 128)])
def test_longform_joint_mode(ctx, sd, engines, B, T, window, overlap):
    """sample_long(mode="joint"): the windows agree bit for bit in every overlap - the last window's long one included -, the stitch holds
    every window on its own span, and the default mode is untouched: its digest after the joint calls is what it was before"""
    eng = _fresh(ctx, sd, engines)
    inp = clip_batch(B, T, 16)
    idx, dts = vm.euler_tables(4)
    args = (eng, inp["x_latent"], inp["t5_cond"], inp["t5_uncond"], inp["midi"], inp["beats"], idx, dts, 3.0)
    kw = dict(window=window, overlap=overlap, seed=3, clip_base=1)
    xf = longform.sample_long(*args, **kw)
    before = _digest(xf)
    z, parts = longform.sample_long(*args, mode="joint", return_windows=True, **kw)
    torch.cuda.synchronize()
    assert z.shape == (B, 20, T) and torch.isfinite(z).all()
    plan = longform.plan_windows(T, window, overlap)
    cont = longform.plan_continue(plan)
    nw = len(plan)
    assert len(parts) == nw and nw >= 3 and cont[-1][2] > overlap, "the case must have a last window that reaches back further"
    for w, (s, n, known) in enumerate(cont):
        assert tuple(parts[w].shape) == (B, 20, n)
        assert torch.equal(z[:, :, s:s + n], parts[w]), f"window {w} is not what the stitch holds on [{s}, {s + n})"
        if w:
            ps, pn, _ = cont[w - 1]
            assert known == ps + pn - s
            assert torch.equal(parts[w - 1][:, :, pn - known:], parts[w][:, :, :known]), f"windows {w - 1} / {w} disagree in their {known} shared tokens"
    assert not torch.equal(z, xf), "joint mode returned the cross-fade result"
    assert torch.equal(z, longform.sample_long(*args, mode="joint", **kw)), "two joint calls (the second may replay a graph)"
    after = _digest(longform.sample_long(*args, **kw))
    assert after == before, "cross-fade mode changed after joint calls"
