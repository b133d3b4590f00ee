"""Per-step guidance weights on the GPU (vb_sample_cfg_sched, through the C ABI): a step of weight 1 is today's step, a step of weight 0
evaluates the conditional branch alone (the n_branch == 1 update), any other weight w runs both branches under the effective scale
fmaf(w, s - 1, 1) - with a scalar scale, per-row scales, a known region and joint windows.

The trajectory is compared with a CPU restatement over oracle.ref_cpu.dit_forward at the sampler's bound, rel-L2 1e-3 per state with equal
routing (tests/test_gpu_joint.py::test_trajectory_follows_the_cpu_restatement).  Everything else is bit for bit (torch.equal): the kinds of
step share one update function (common.h:euler_cfg_update), a clip's evaluation does not depend on its batch slot, and the router noise of
the conditional rows is keyed as in a two-branch step whatever the schedule."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, clip_batch, describe, exp_noise, gumbel_arrays, gumbel_arrays_steps, rel_l2
from versband_amd import _lib as L
from versband_amd import model as vm
from versband_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 1e-4
ALL_ONE = 2e-7          # of the tensor's max-abs (tests/test_gpu_joint.py)
B, T, LC = 2, 40, 8
MIXED = [0.0, 1.0, 0.5, 0.0, 1.0, 0.25]       # all three kinds of step, every change between them
ROW_SCALES = [1.5, 4.5]
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


@pytest.fixture(scope="module")
def inp():
    return clip_batch(B, T, LC)


def _cond(eng, inp, T, nb=2, t5_uncond=None):
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"] if t5_uncond is None else t5_uncond]) if nb == 2 else inp["t5_cond"]
    return eng.precompute_cond(t5, inp["midi"], inp["beats"], T)


@pytest.fixture
def knobs(monkeypatch):
    """set VB_* knobs for a while: knobs(VB_X="1") ... knobs() restores; the library's cached tuning never outlives the test"""
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


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("form,T1", [("scalar", 40), ("rows", 37)])
def test_trajectory_follows_the_cpu_restatement(engines, sd, form, T1):
    """split precision, injected router noise, 6 steps under [0, 1, 0.5, 0, 1, 0.25]: every state against ref_cpu.dit_forward per branch
    + the step's update - the conditional branch alone at weight 0, s_k = 1 + w (s - 1) elsewhere - with equal routing at every state.
    Per-row scales run at T = 37: a wave of the fused launch then holds the last token of clip 0 and the first of clip 1."""
    eng = engines["split"]
    cfg = synth.DiTConfig()
    inp = clip_batch(B, T1, LC)
    timesteps = len(MIXED) + 1
    idx, dts = vm.euler_tables(timesteps)
    steps = len(idx)
    E, depth = cfg.num_experts, cfg.depth
    scale = 3.0 if form == "scalar" else ROW_SCALES
    noise_steps = [[exp_noise(B, T1, E, 2 * k + br, depth) for br in (0, 1)] for k in range(steps)]
    cond = _cond(eng, inp, T1)
    x, traj = eng.sample_cfg(inp["x_latent"], cond, idx, dts, scale, noise=gumbel_arrays_steps(noise_steps), return_traj=True, guidance=MIXED)
    torch.cuda.synchronize()
    traj = traj.cpu()
    assert torch.equal(x.cpu(), traj[-1]) and torch.isfinite(traj).all() and torch.equal(traj[0], inp["x_latent"])
    cc = ref_cpu.dit_precompute(sd, inp["t5_cond"], inp["midi"], inp["beats"], T1)
    cu = ref_cpu.dit_precompute(sd, inp["t5_uncond"], inp["midi"], inp["beats"], T1)
    t_span, tidx = ref_cpu.t_index_table(timesteps, None)
    s = torch.full((B, 1, 1), 3.0) if form == "scalar" else torch.tensor(ROW_SCALES).reshape(B, 1, 1)
    xr = inp["x_latent"].clone()
    want, routes = [xr.clone()], []
    t = t_span[0]
    for k in range(steps):
        dt = t_span[k + 1] - t
        ti = torch.full((B,), tidx[k], dtype=torch.long)
        e_c, aux_c = ref_cpu.dit_forward(sd, xr, ti, cc, noise_steps[k][0], return_aux=True)
        if MIXED[k] == 0.0:
            xr = xr + dt * e_c
            routes.append((aux_c, None))
        else:
            e_u, aux_u = ref_cpu.dit_forward(sd, xr, ti, cu, noise_steps[k][1], return_aux=True)
            sk = 1.0 + MIXED[k] * (s - 1.0)
            xr = xr + dt * (e_u + sk * (e_c - e_u))
            routes.append((aux_c, aux_u))
        t = t + dt
        want.append(xr.clone())
    for k in range(steps + 1):
        err = rel_l2(traj[k], want[k])
        print(f"guidance schedule, {form}, state {k}: rel_l2 = {err:.3e} (bound 1e-3)")
        assert err < 1e-3, describe(f"{form}: state {k} vs restatement", traj[k], want[k])
    # routing: the network evaluated at each state of the GPU trajectory routes like the oracle did at its own
    N = B * T1
    for k in range(steps):
        t_idx = torch.full((2 * B,), idx[k], dtype=torch.int64)
        _, got = eng.forward(traj[k], t_idx, cond, noise=gumbel_arrays(noise_steps[k]), return_routes=True)
        torch.cuda.synchronize()
        for br in (0, 1):
            if routes[k][br] is None:
                continue
            for i in range(depth):
                for j, name in ((0, "ic"), (1, "ia")):
                    r_got = got[i, j, br * N:(br + 1) * N].cpu().long()
                    assert torch.equal(r_got, routes[k][br][f"{name}{i}"]), f"step {k} branch {br} block {i} {name} routes differently"


# ---------------------------------------------------------------------------------------------------------------- 2
def test_all_ones_is_the_plain_call(ctx, sd, engines, inp):
    """a schedule of ones takes the plain call's code path and its graph-cache entry: equal bits, no new graph"""
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(5)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).cuda()
    midi, beats, x0 = inp["midi"].cuda(), inp["beats"].cuda(), inp["x_latent"].cuda()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
        plain = [eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=5) for _ in range(2)]
        stream.synchronize()
        assert eng.graphs() == 1
        ones = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=5, guidance=[1.0] * 4)
        # ... and through the new entry point itself, past the host's shortcut
        gs = L.Guidance((C.c_float * 4)(1.0, 1.0, 1.0, 1.0))
        x = x0.clone()
        tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
        ns = L.Noise(None, None, None, 5, 0, 0)
        rc = eng.ctx.lib.vb_sample_cfg_sched(eng.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, 2, T, LC, 4, L.ptr(tt), L.ptr(dd), 3.0, C.byref(gs),
                                             None, None, None, C.byref(ns), None, L.ptr(eng._workspace(B, 2, T, LC)), L.stream_ptr())
        stream.synchronize()
        assert rc == 0, eng.ctx.lib.vb_last_error()
        assert eng.graphs() == 1, "all ones must replay the plain call's graph"
    assert torch.isfinite(plain[0]).all() and torch.equal(plain[0], plain[1])
    assert torch.equal(ones, plain[0]), describe("all ones vs the plain call", ones, plain[0])
    assert torch.equal(x, plain[0]), describe("all ones through vb_sample_cfg_sched vs the plain call", x, plain[0])


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_all_zeros_is_the_one_branch_call(engines, inp, prec):
    """every step single-branch, in the two-branch layout, against an n_branch = 1 call on conditioning precomputed for the conditional
    branch alone: same seed and clip ids, and the same evaluation indices - an n_branch = 1 call keys step k's noise (seed, clip, k,
    branch 0), which is what the conditional rows of a two-branch step draw"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(5)
    zeros, tz = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 2), idx, dts, 3.0, seed=5, clip_base=3, guidance=[0.0] * 4, return_traj=True)
    one, t1 = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 1), idx, dts, 1.0, seed=5, clip_base=3, return_traj=True)
    guided = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 2), idx, dts, 3.0, seed=5, clip_base=3)
    torch.cuda.synchronize()
    print(f"all zeros vs n_branch = 1, {prec}: rel_l2 = {rel_l2(zeros, one):.3e}, equal = {torch.equal(zeros, one)}")
    assert torch.isfinite(zeros).all() and not torch.equal(zeros, guided)
    for k in range(5):
        assert torch.equal(tz[k], t1[k]), describe(f"{prec}: all zeros vs the n_branch = 1 call, state {k}", tz[k], t1[k])
    assert torch.equal(zeros, one)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_single_branch_steps_do_not_see_the_unconditional_rows(engines, inp):
    """two calls that differ in the unconditional T5 embedding only: equal under an all-zero schedule; under [0, 0, 1, 1] equal through
    state 2 and different after it"""
    eng = engines["bf16"]
    idx, dts = vm.euler_tables(5)
    other = torch.randn(inp["t5_uncond"].shape, generator=torch.Generator().manual_seed(77))
    out = {}
    for name, tu in (("a", None), ("b", other)):
        cond = _cond(eng, inp, T, 2, tu)
        out[name, "zeros"] = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=5, guidance=[0.0] * 4)
        out[name, "half"] = eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=5, guidance=[0.0, 0.0, 1.0, 1.0], return_traj=True)[1]
    torch.cuda.synchronize()
    assert torch.isfinite(out["a", "zeros"]).all() and torch.equal(out["a", "zeros"], out["b", "zeros"])
    ta, tb = out["a", "half"], out["b", "half"]
    for k in range(3):
        assert torch.equal(ta[k], tb[k]), describe(f"state {k} under [0, 0, 1, 1]", ta[k], tb[k])
    assert not torch.equal(ta[3], tb[3]) and not torch.equal(ta[4], tb[4]), "the guided steps must see the unconditional rows"


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("prec", ["bf16", "split"])
@pytest.mark.parametrize("form", ["scalar", "rows", "rows_keep"])
def test_fused_update_equals_the_separate_launches(engines, knobs, prec, form):
    """VB_EULER_LAUNCH=1 under the mixed schedule: the scheduled instances of the fused FinalLayer and of the separate update are one
    device function.  T = 37: a wave's two tokens belong to two clips."""
    eng = engines[prec]
    T1 = 37
    inp = clip_batch(B, T1, LC)
    idx, dts = vm.euler_tables(len(MIXED) + 1)
    x0 = inp["x_latent"]
    mask = torch.zeros(B, T1)
    mask[0, :10] = 1.0
    mask[1, 30:33] = torch.tensor([0.75, 0.5, 0.25])
    keep = (torch.randn(x0.shape, generator=torch.Generator().manual_seed(5)), x0, mask, vm.euler_times(len(MIXED) + 1), SIGMA) if form == "rows_keep" else None
    scale = 3.0 if form == "scalar" else ROW_SCALES
    outs = []
    for knob in ({}, {"VB_EULER_LAUNCH": "1"}):
        knobs(**knob)
        outs.append(eng.sample_cfg(x0, _cond(eng, inp, T1), idx, dts, scale, seed=21, keep=keep, guidance=MIXED, return_traj=True)[1].clone())
        torch.cuda.synchronize()
    knobs()
    assert torch.isfinite(outs[0]).all()
    for k in range(len(MIXED) + 1):
        assert torch.equal(outs[0][k], outs[1][k]), describe(f"{form} {prec}: fused vs separate launches, state {k}", outs[1][k], outs[0][k])
    plain = eng.sample_cfg(x0, _cond(eng, inp, T1), idx, dts, scale, seed=21, keep=keep)
    torch.cuda.synchronize()
    assert not torch.equal(plain, outs[0][-1]), "the schedule was not read"


# ---------------------------------------------------------------------------------------------------------------- 6
def test_graph_replay_equals_eager_and_keys_on_the_weights(ctx, sd, engines, inp, knobs):
    """calls two and three replay one graph; another schedule of the same length captures a second; rewriting the per-row scales in place
    replays the first; a new seed replays and matches its eager result"""
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(len(MIXED) + 1)
    other = [1.0, 0.0, 0.0, 2.0, 0.5, 1.0]
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).cuda()
    midi, beats, x0 = inp["midi"].cuda(), inp["beats"].cuda(), inp["x_latent"].cuda()
    scale_t = torch.tensor(ROW_SCALES, device="cuda")
    stream = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
        for rep in range(3):                         # eager, capture + replay, replay
            out["a", rep] = eng.sample_cfg(x0, cond, idx, dts, scale_t, seed=7 + rep, guidance=MIXED)
        stream.synchronize()
        assert eng.graphs() == 1, "the repeated scheduled call was not captured, or each call captured its own graph"
        for rep in range(2):
            out["b", rep] = eng.sample_cfg(x0, cond, idx, dts, scale_t, seed=7 + rep, guidance=other)
        stream.synchronize()
        assert eng.graphs() == 2, "another schedule must capture its own graph"
        scale_t.copy_(torch.tensor([2.0, 1.25]))
        out["c", 0] = eng.sample_cfg(x0, cond, idx, dts, scale_t, seed=7, guidance=list(MIXED))
        stream.synchronize()
        assert eng.graphs() == 2, "rewritten row scales replay the first graph"
        for rep in range(2):
            out["s", rep] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7 + rep, guidance=MIXED)
        out["p", 0] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7)
        out["p", 1] = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=7)
        stream.synchronize()
        assert eng.graphs() == 4, "the scalar scheduled call and the plain call have their own graphs"
    knobs(VB_NO_GRAPH="1")
    eager = _fresh(ctx, sd, engines)
    with torch.cuda.stream(stream):
        cond = eager.precompute_cond(t5, midi, beats, T, persistent=True)
        cases = [(("a", r), ROW_SCALES, 7 + r, MIXED) for r in range(3)] + [(("b", r), ROW_SCALES, 7 + r, other) for r in range(2)]
        cases += [(("c", 0), [2.0, 1.25], 7, MIXED)] + [(("s", r), 3.0, 7 + r, MIXED) for r in range(2)] + [(("p", r), 3.0, 7, None) for r in range(2)]
        for key, s, seed, g in cases:
            want = eager.sample_cfg(x0, cond, idx, dts, s, seed=seed, guidance=g)
            stream.synchronize()
            assert torch.isfinite(want).all() and torch.equal(out[key], want), describe(f"graph vs eager, {key}", out[key], want)
    assert eager.graphs() == 0
    assert not torch.equal(out["a", 0], out["a", 1]) and not torch.equal(out["a", 0], out["b", 0]) and not torch.equal(out["a", 0], out["c", 0])


# ---------------------------------------------------------------------------------------------------------------- 7
BC, T_LONG, WIN = 2, 100, 40
STARTS = (0, 32, 60)
NW = len(STARTS)


def _rows(inp, clips=slice(None)):
    """the rows sample_long builds for the plan (tests/test_gpu_joint.py): row = w * Bc + b"""
    x = torch.cat([inp["x_latent"][clips, :, s:s + WIN] for s in STARTS]).contiguous()
    midi = torch.cat([inp["midi"][clips][..., 2 * s:2 * (s + WIN)] for s in STARTS]).contiguous()
    beats = torch.cat([inp["beats"][clips][..., 2 * s:2 * (s + WIN)] for s in STARTS]).contiguous()
    return x, midi, beats, torch.cat([inp["t5_cond"][clips].repeat(NW, 1, 1), inp["t5_uncond"][clips].repeat(NW, 1, 1)])


def _assert_overlaps_agree(x, what):
    n = x.shape[-1]
    for w in range(NW - 1):
        ov = STARTS[w] + n - STARTS[w + 1]
        a, b = x[w * BC:(w + 1) * BC, :, n - ov:], x[(w + 1) * BC:(w + 2) * BC, :, :ov]
        assert torch.equal(a, b), describe(f"{what}: overlap of windows {w} / {w + 1} ({ov} tokens)", a, b)


def _path(t, ref, x0, sigma=SIGMA):
    """r(t) on the host in float32 (tests/test_gpu_joint.py)"""
    t = np.float32(t)
    c0 = np.float32(1) - np.float32(np.float32(1) - np.float32(sigma)) * t
    return torch.from_numpy((t * ref.numpy().astype(np.float32) + np.float32(c0) * x0.numpy().astype(np.float32)).astype(np.float32))


def test_schedule_with_a_known_region_and_joint_windows(engines):
    """keep + windows under the mixed schedule: the overlaps agree bit for bit in every state, the masked tokens sit on the path after
    every step - single-branch ones included - and a clip does not depend on its neighbour in the batch"""
    eng = engines["bf16"]
    long = clip_batch(BC, T_LONG, LC)
    idx, dts = vm.euler_tables(len(MIXED) + 1)
    times = vm.euler_times(len(MIXED) + 1)
    Bw = NW * BC
    x, midi, beats, t5 = _rows(long)
    ref = torch.randn(x.shape, generator=torch.Generator().manual_seed(6))
    mask = torch.zeros(Bw, WIN)
    mask[:BC, :12] = 1.0
    base = 2 * NW
    cond = eng.precompute_cond(t5, midi, beats, WIN)
    got, traj = eng.sample_cfg(x, cond, idx, dts, 3.0, seed=9, clip_base=base, windows=STARTS, keep=(ref, x, mask, times, SIGMA), guidance=MIXED,
                               return_traj=True)
    plain = eng.sample_cfg(x, cond, idx, dts, 3.0, seed=9, clip_base=base, windows=STARTS, keep=(ref, x, mask, times, SIGMA))
    torch.cuda.synchronize()
    traj = traj.cpu()
    assert torch.isfinite(traj).all() and not torch.equal(got, plain)
    for k in range(len(idx)):
        have, want = traj[k + 1][:BC, :, :12], _path(times[k], ref, x)[:BC, :, :12]
        err, mx = float((have - want).abs().max()), float(want.abs().max())
        print(f"kept tokens after step {k} (weight {MIXED[k]}): max|diff| = {err / mx:.3e} of max-abs (bound {ALL_ONE:.0e})")
        assert err <= ALL_ONE * mx
        _assert_overlaps_agree(traj[k + 1], f"schedule + joint + keep, traj[{k + 1}]")
    for b in range(BC):
        x1, midi1, beats1, t51 = _rows(long, clips=slice(b, b + 1))
        cond1 = eng.precompute_cond(t51, midi1, beats1, WIN)
        k1 = (ref[b::BC].contiguous(), x1, mask[b::BC].contiguous(), times, SIGMA)
        alone = eng.sample_cfg(x1, cond1, idx, dts, 3.0, seed=9, clip_ids=[base + w * BC + b for w in range(NW)], windows=STARTS, keep=k1,
                               guidance=MIXED)
        torch.cuda.synchronize()
        assert torch.equal(alone, got[b::BC]), describe(f"clip {b} alone vs beside its neighbour", alone, got[b::BC])


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("bad,at", [([1.0, float("nan"), 0.0, 1.0], 1), ([-0.25, 1.0, 1.0, 1.0], 0), ([1.0, 1.0, 1.0, 16.5], 3),
                                    ([1.0, 0.0, float("inf"), 1.0], 2)])
def test_invalid_schedules_are_refused_before_any_launch(ctx, sd, engines, inp, bad, at):
    """NaN, negative, above 16, infinite: VB_E_INVALID with the step named, the state untouched and no graph made"""
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(5)
    cond = _cond(eng, inp, T, 2)
    x0 = inp["x_latent"].cuda()
    x = x0.clone()
    tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
    ns = L.Noise(None, None, None, 5, 0, 0)
    gs = L.Guidance((C.c_float * 4)(*bad))
    ws = eng._workspace(B, 2, T, LC)
    rc = eng.ctx.lib.vb_sample_cfg_sched(eng.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, 2, T, LC, 4, L.ptr(tt), L.ptr(dd), 3.0, C.byref(gs), None, None,
                                         None, C.byref(ns), None, L.ptr(ws), L.stream_ptr())
    msg = eng.ctx.lib.vb_last_error().decode()
    torch.cuda.synchronize()
    assert rc == VB_E_INVALID and f"weight[{at}]" in msg, (rc, msg)
    assert torch.equal(x, x0) and eng.graphs() == 0
    with pytest.raises(ValueError, match=rf"guidance\[{at}\]"):
        eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, guidance=bad)
    with pytest.raises(ValueError, match="3 entries for 4 steps"):
        eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, guidance=[1.0, 0.0, 1.0])
    # with one branch there is nothing to guide: the schedule is not read
    x1 = x0.clone()
    cond1 = _cond(eng, inp, T, 1)
    rc = eng.ctx.lib.vb_sample_cfg_sched(eng.ctx.handle, L.ptr(x1), L.ptr(cond1["buf"]), B, 1, T, LC, 4, L.ptr(tt), L.ptr(dd), 3.0, C.byref(gs), None, None,
                                         None, C.byref(ns), None, L.ptr(eng._workspace(B, 1, T, LC)), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(x1).all() and not torch.equal(x1, x0)


# ---------------------------------------------------------------------------------------------------------------- 9
def test_cli_interval_over_every_step_writes_the_same_files(tmp_path):
    """scripts/infer_batched.py --synthetic 2 --guidance_interval 0-1 covers every step: the files of the run without the flag, byte for
    byte (that the flag reaches the sampler is tests/test_guidance_host.py's)"""
    common = [sys.executable, os.path.join(ROOT, "scripts", "infer_batched.py"), "--synthetic", "2", "--synthetic_frames", "150", "--ddim_steps", "3",
              "--scales", "1-3", "--n_samples", "1", "--items_per_batch", "2"]
    listing = {}
    for name, extra in (("plain", []), ("all", ["--guidance_interval", "0-1"])):
        out = tmp_path / "gen"                       # the same save_dir for both runs: clap.csv holds the paths
        r = subprocess.run(common + extra + ["--save_dir", str(out)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {}
        for d, _, names in os.walk(out):
            for nm in names:
                if nm.endswith(".wav") or nm == "clap.csv":
                    p = os.path.join(d, nm)
                    files[os.path.relpath(p, out)] = open(p, "rb").read()
                    os.remove(p)
        listing[name] = files
    want = listing["plain"]
    assert len([f for f in want if f.endswith(".wav")]) == 2 * 2 and sorted(listing["all"]) == sorted(want)
    for f in sorted(want):
        assert listing["all"][f] == want[f], f"{f}: --guidance_interval 0-1 differs from the run without the flag"
