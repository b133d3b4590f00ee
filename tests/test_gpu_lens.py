"""Clips of different lengths as rows of one call on the GPU (vb_lens: vb_attention_lens, vb_dit_precompute_cond_lens,
vb_dit_forward_lens, vb_sample_cfg_lens).  THE CONTRACT: a row of a call with lengths is the call on that clip alone.

Every comparison here is bit for bit (torch.equal) on the valid tokens.  Row lengths [200, 128, 65, 40] at T = 200: a full row, an end
exactly on a 64-key tile boundary, one key in the last tile with the second 128-query workgroup wholly padding, less than one key tile."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests.helpers import SEED, describe, rel_l2
from versband_amd import _lib as L
from versband_amd import harness
from versband_amd import model as vm
from versband_amd import pack, prng, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LC, LENS = 200, 8, [200, 128, 65, 40]
B = len(LENS)
CLIPS = [7, 2, 9, 4]
SIGMA = 1e-4


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
    return torch.from_numpy(prng.normal(prng.key_seed(11, name), int(np.prod(shape))).reshape(shape)).float() * scale


@pytest.fixture(scope="module")
def batch():
    """the four clips alone (clip b has LENS[b] tokens and 2 LENS[b] midi / beats frames) and as rows padded to T: the padding of x
    is finite noise, that of midi / beats index 0"""
    alone = [synth.make_clip_inputs(SEED, b, n, L=LC) for b, n in enumerate(LENS)]
    x = _rnd((B, 20, T), "xpad", 0.5)
    midi, beats = torch.zeros(B, 2 * T, dtype=torch.int64), torch.zeros(B, 2 * T, dtype=torch.int64)
    for b, (c, n) in enumerate(zip(alone, LENS)):
        x[b, :, :n] = c["x_latent"]
        midi[b, :2 * n] = c["midi"].reshape(-1)
        beats[b, :2 * n] = c["beats"].reshape(-1)
    return {"alone": alone, "x": x, "midi": midi, "beats": beats,
            "t5_cond": torch.stack([c["t5_cond"] for c in alone]), "t5_uncond": torch.stack([c["t5_uncond"] for c in alone])}


def _cond(eng, bt, nb=2, lengths=LENS, midi=None, beats=None):
    t5 = torch.cat([bt["t5_cond"], bt["t5_uncond"]]) if nb == 2 else bt["t5_cond"]
    return eng.precompute_cond(t5, bt["midi"] if midi is None else midi, bt["beats"] if beats is None else beats, T, lengths=lengths)


def _cond_alone(eng, bt, b, nb=2):
    c = bt["alone"][b]
    t5 = torch.stack([c["t5_cond"], c["t5_uncond"]]) if nb == 2 else c["t5_cond"][None]
    return eng.precompute_cond(t5, c["midi"], c["beats"], LENS[b])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("npl", [1, 2])
def test_attention_rows_equal_the_attention_of_the_clip_alone(npl):
    """vb_attention_lens: row b's first len[b] output rows equal vb_attention on that row's tokens alone (T = len[b], its own Tpad, V^T
    planes cleared) bit for bit and are within test_attention's tolerance of the float64 reference; the padding rows are finite"""
    lib = L.load()
    H, hd, Lc = 2, 96, 80
    q, k, v = _rnd((B, T, H, hd), "aq"), _rnd((B, T, H, hd), "ak"), _rnd((B, T, H, hd), "av")
    ky, vy, cw = _rnd((B, Lc, H, hd), "aky"), _rnd((B, Lc, H, hd), "avy"), _rnd((H,), "acw")

    def vt_layout(x, S, Spad):   # [b,S,H,hd] -> [b,H,hd,Spad] zero padded
        o = torch.zeros(x.shape[0], H, hd, Spad)
        o[..., :S] = x.permute(0, 2, 3, 1)
        return o

    def run(qq, kk, vv, kyy, vyy, t, lens):
        tpad, lpad = (t + 63) // 64 * 64, (Lc + 63) // 64 * 64
        nb = qq.shape[0]
        planes = [pack.to_planes(a, npl).cuda().contiguous() for a in (qq, kk, vt_layout(vv, t, tpad), kyy, vt_layout(vyy, Lc, lpad))]
        cwd = cw.cuda()
        out = torch.full((npl, nb, t, H, hd), float("nan"), dtype=torch.bfloat16, device="cuda")
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda") if lens is not None else None
        fn = lib.vb_attention_lens if lens is not None else lib.vb_attention
        extra = (L.ptr(ld),) if lens is not None else ()
        L.check(fn(*[L.ptr(p) for p in planes], L.ptr(cwd), nb, t, tpad, Lc, lpad, H, hd, npl, *extra, L.ptr(out), L.stream_ptr()), "attention")
        torch.cuda.synchronize()
        return out.cpu(), planes

    got, planes = run(q, k, v, ky, vy, T, LENS)
    assert torch.isfinite(got.float()).all(), "a padding row of the output is not finite (or was not written)"
    tol = 6e-3 if npl == 1 else 4e-5
    src = (lambda t, pl: pack.planes_to_float(pl.cpu()).reshape(t.shape)) if npl == 1 else (lambda t, pl: t)
    qq, kk, kyy = src(q, planes[0]).double(), src(k, planes[1]).double(), src(ky, planes[3]).double()
    vv, vyy = (v.to(torch.bfloat16).double(), vy.to(torch.bfloat16).double()) if npl == 1 else (v.double(), vy.double())
    for b, n in enumerate(LENS):
        sel = slice(b, b + 1)
        want, _ = run(q[sel, :n].contiguous(), k[sel, :n].contiguous(), v[sel, :n].contiguous(), ky[sel], vy[sel], n, None)
        assert torch.equal(got[:, b, :n].view(torch.int16), want[:, 0].view(torch.int16)), \
            describe(f"np={npl} row {b} (len {n}) vs the clip alone", pack.planes_to_float(got[:, b:b + 1, :n]), pack.planes_to_float(want))
        p = lambda t: t[sel, :n].permute(0, 2, 1, 3)
        ref = ref_cpu.sdpa(p(qq), p(kk), p(vv)) + ref_cpu.sdpa(p(qq), kyy[sel].permute(0, 2, 1, 3), vyy[sel].permute(0, 2, 1, 3)) * cw.double().view(1, H, 1, 1)
        g = pack.planes_to_float(got[:, b:b + 1, :n])
        err = rel_l2(g, ref.permute(0, 2, 1, 3))
        print(f"attention_lens np={npl} row {b} len {n}: rel_l2 {err:.3e} (tol {tol:g})")
        assert err < tol, describe(f"attention_lens np={npl} row {b}", g, ref.permute(0, 2, 1, 3))


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_forward_rows_equal_the_forward_of_the_clip_alone(engines, batch, prec):
    """vb_dit_forward_lens after vb_dit_precompute_cond_lens: v_out[b][:, :len[b]] and route_out on the valid tokens equal the B = 1,
    T = len[b] precompute + forward"""
    eng = engines[prec]
    depth = synth.DiTConfig().depth
    t_idx = torch.tensor([100, 300, 500, 700] * 2)
    v, routes = eng.forward(batch["x"], t_idx, _cond(eng, batch), seed=5, clip_base=3, return_routes=True, lengths=LENS)
    torch.cuda.synchronize()
    v, routes = v.cpu().view(2, B, 20, T), routes.cpu().view(depth, 2, 2, B, T)
    assert torch.isfinite(v).all(), "padding tokens of v_out must stay finite"
    for b, n in enumerate(LENS):
        va, ra = eng.forward(batch["alone"][b]["x_latent"][None], t_idx[[b, B + b]], _cond_alone(eng, batch, b), seed=5, clip_base=3 + b, return_routes=True)
        torch.cuda.synchronize()
        va, ra = va.cpu().view(2, 20, n), ra.cpu().view(depth, 2, 2, n)
        assert torch.equal(routes[:, :, :, b, :n], ra), f"{prec} row {b}: {int((routes[:, :, :, b, :n] != ra).sum())} routes differ from the clip alone"
        assert torch.equal(v[:, b, :, :n], va), describe(f"{prec} row {b} (len {n}): v_out vs the clip alone", v[:, b, :, :n], va)


# ---------------------------------------------------------------------------------------------------------------- 3
def _alone_traj(eng, batch, b, idx, dts, scale, **kw):
    return eng.sample_cfg(batch["alone"][b]["x_latent"][None], _cond_alone(eng, batch, b), idx, dts, scale, seed=5, clip_base=CLIPS[b], return_traj=True, **kw)


@pytest.fixture(scope="module")
def alone_trajs(engines, batch):
    """the 3-step trajectories of the four clips alone, per precision: computed once, shared, left unchanged"""
    idx, dts = vm.euler_tables(4)
    out = {}
    for prec in ("bf16", "split"):
        out[prec] = [_alone_traj(engines[prec], batch, b, idx, dts, 3.0)[1].cpu() for b in range(B)]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("prec", ["bf16", "split"])
@pytest.mark.parametrize("launch", ["fused", "VB_EULER_LAUNCH"])
def test_sampler_rows_equal_the_sampler_call_of_the_clip_alone(engines, batch, alone_trajs, knobs, prec, launch):
    """3 steps through vb_sample_cfg_lens: every traj[k][b][:, :len[b]] and the result equal the alone call's, in the fused update and
    with VB_EULER_LAUNCH=1"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    if launch != "fused":
        knobs(**{launch: "1"})
    x, traj = eng.sample_cfg(batch["x"], _cond(eng, batch), idx, dts, 3.0, seed=5, clip_ids=CLIPS, return_traj=True, lengths=LENS)
    torch.cuda.synchronize()
    x, traj = x.cpu(), traj.cpu()
    assert torch.isfinite(traj).all()
    for b, n in enumerate(LENS):
        want = alone_trajs[prec][b]
        for k in range(4):
            assert torch.equal(traj[k, b, :, :n], want[k, 0]), describe(f"{prec} {launch} row {b} (len {n}) state {k}", traj[k, b, :, :n], want[k, 0])
        assert torch.equal(x[b, :, :n], want[3, 0])
        assert not x[b, :, n:].any(), "the host zero-fills the padding of the returned latent"


def test_sampler_graph_replay_equals_the_eager_call(ctx, sd, engines, batch, alone_trajs):
    """the third call with the same lengths replays a captured graph and gives the bits of the eager first call - those of the clips alone"""
    eng = _fresh(ctx, sd, engines)
    idx, dts = vm.euler_tables(4)
    stream = torch.cuda.Stream()
    dev = {k: batch[k].cuda() for k in ("x", "midi", "beats", "t5_cond", "t5_uncond")}
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(torch.cat([dev["t5_cond"], dev["t5_uncond"]]), dev["midi"], dev["beats"], T, persistent=True, lengths=LENS)
        outs = [eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, seed=5, clip_ids=CLIPS, lengths=LENS).cpu() for _ in range(3)]
        stream.synchronize()
    assert eng.graphs() == 1, "the repeated lengths call was not captured"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), describe("graph replay vs the eager first call", outs[2], outs[0])
    for b, n in enumerate(LENS):
        assert torch.equal(outs[2][b, :, :n], alone_trajs["bf16"][b][3, 0])


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_padding_is_never_read(engines, batch, prec):
    """the same call twice; the second has the padding of x at 1e30 in one row and NaN in another, and that of midi / beats at other valid
    indices: the valid regions are bit-identical (the same launches run on both sides).  Fails without the proj_in / stem masking."""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    _, first = eng.sample_cfg(batch["x"], _cond(eng, batch), idx, dts, 3.0, seed=5, clip_ids=CLIPS, return_traj=True, lengths=LENS)
    first = first.cpu()
    x, midi, beats = batch["x"].clone(), batch["midi"].clone(), batch["beats"].clone()
    x[1, :, LENS[1]:] = 1e30
    x[2, :, LENS[2]:] = float("nan")
    x[3, :, LENS[3]:] = -7.0
    for b, n in enumerate(LENS):
        midi[b, 2 * n:] = 57 + b
        beats[b, 2 * n:] = 1 + b % 2
    _, second = eng.sample_cfg(x, _cond(eng, batch, midi=midi, beats=beats), idx, dts, 3.0, seed=5, clip_ids=CLIPS, return_traj=True, lengths=LENS)
    torch.cuda.synchronize()
    second = second.cpu()
    for b, n in enumerate(LENS):
        assert torch.isfinite(second[:, b, :, :n]).all(), f"row {b}: the padding reached a valid token"
        assert torch.equal(first[:, b, :, :n], second[:, b, :, :n]), describe(f"{prec} row {b}: other padding, other result", second[:, b, :, :n], first[:, b, :, :n])


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("prec", ["bf16", "split"])
def test_lengths_compose_with_rows_keep_and_guidance(engines, batch, prec):
    """one call with per-row scales, a known region whose mask covers tokens on both sides of len[b] - 1, and a schedule with a 0, a 1 and a
    0.5 step, against the alone calls with the same blocks sliced"""
    eng = engines[prec]
    idx, dts = vm.euler_tables(4)
    times = vm.euler_times(4)
    scales, sched = [1.5, 3.0, 4.5, 2.0], [0.0, 1.0, 0.5]
    ref = _rnd((B, 20, T), "keep_ref")
    mask = torch.zeros(B, T)
    for b, n in enumerate(LENS):
        mask[b, n - 6:min(T, n + 6)] = 1.0                    # both sides of the clip's last token
        mask[b, n - 9:n - 6] = torch.tensor([0.25, 0.5, 0.75])
    keep = (ref, batch["x"], mask, times, SIGMA)
    _, traj = eng.sample_cfg(batch["x"], _cond(eng, batch), idx, dts, scales, seed=5, clip_ids=CLIPS, return_traj=True, lengths=LENS, keep=keep, guidance=sched)
    torch.cuda.synchronize()
    traj = traj.cpu()
    for b, n in enumerate(LENS):
        sel = slice(b, b + 1)
        k1 = (ref[sel, :, :n].contiguous(), batch["x"][sel, :, :n].contiguous(), mask[sel, :n].contiguous(), times, SIGMA)
        _, want = _alone_traj(eng, batch, b, idx, dts, scales[b], keep=k1, guidance=sched)
        torch.cuda.synchronize()
        want = want.cpu()
        for k in range(4):
            assert torch.equal(traj[k, b, :, :n], want[k, 0]), describe(f"{prec} composed row {b} (len {n}) state {k}", traj[k, b, :, :n], want[k, 0])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_graphs_and_forwarding(ctx, sd, engines, batch):
    """lens = all T and lens = NULL give the bits of vb_sample_cfg_sched and add no graph; two different length sets on the same buffers
    hold two graphs; a plain call afterwards replays the plain one"""
    eng = _fresh(ctx, sd, engines)
    lib = eng.ctx.lib
    idx, dts = vm.euler_tables(4)
    stream = torch.cuda.Stream()
    dev = {k: batch[k].cuda() for k in ("x", "midi", "beats", "t5_cond", "t5_uncond")}
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(torch.cat([dev["t5_cond"], dev["t5_uncond"]]), dev["midi"], dev["beats"], T, persistent=True)
        # vb_sample_cfg_sched itself, on buffers of its own (eager: its key is seen once)
        xs = dev["x"].clone()
        tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
        ns = L.Noise()
        ns.seed, ns.clip_base, ns.nfe = 5, 0, 0
        L.check(lib.vb_sample_cfg_sched(eng.ctx.handle, L.ptr(xs), L.ptr(cond["buf"]), B, 2, T, LC, 3, L.ptr(tt), L.ptr(dd), 3.0, None, None, None, None,
                                        C.byref(ns), None, L.ptr(eng._workspace(B, 2, T, LC)), L.stream_ptr()), "vb_sample_cfg_sched")
        stream.synchronize()
        plain = [eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, seed=5).cpu() for _ in range(2)]
        stream.synchronize()
        assert eng.graphs() == 1
        full = eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, seed=5, lengths=[T] * B).cpu()
        stream.synchronize()
        assert eng.graphs() == 1, "lengths that all equal T must replay the plain graph"
        assert torch.equal(plain[0], xs.cpu()) and torch.equal(plain[1], xs.cpu()) and torch.equal(full, xs.cpu())
        # (the conditioning was made without lengths: this part counts graphs and compares a set of lengths with itself)
        sets = [LENS, [190, 64, 200, 1]]
        outs = [[eng.sample_cfg(dev["x"], dict(cond, lengths=tuple(s)), idx, dts, 3.0, seed=5, lengths=s).cpu() for _ in range(3)] for s in sets]
        stream.synchronize()
        assert eng.graphs() == 3, "every set of lengths captures its own graph"
        for o in outs:
            assert torch.equal(o[0], o[1]) and torch.equal(o[0], o[2])
        assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][0][1, :, :LENS[1]], plain[0][1, :, :LENS[1]])
        again = eng.sample_cfg(dev["x"], cond, idx, dts, 3.0, seed=5).cpu()
        stream.synchronize()
        assert eng.graphs() == 3 and torch.equal(again, plain[0]), "a plain call afterwards replays the plain graph"


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals_name_the_row_and_leave_x_unchanged(engines, batch):
    eng = engines["bf16"]
    lib = eng.ctx.lib
    idx, dts = vm.euler_tables(4)
    cond = _cond(eng, batch)
    x = batch["x"].cuda()
    before = x.clone()
    tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
    ws = eng._workspace(B, 2, T, LC)
    ns = L.Noise()

    def sample(lens, win=None):
        arr = (C.c_int32 * B)(*lens)
        ls = L.Lens(arr)
        return lib.vb_sample_cfg_lens(eng.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, 2, T, LC, 3, L.ptr(tt), L.ptr(dd), 3.0, C.byref(ls), None,
                                      C.byref(win) if win is not None else None, None, None, C.byref(ns), None, L.ptr(ws), L.stream_ptr())

    assert sample([200, 0, 65, 40]) == -1 and b"row 1" in lib.vb_last_error()
    assert sample([200, 128, 201, 40]) == -1 and b"row 2" in lib.vb_last_error()
    starts = (C.c_int32 * 2)(0, 150)
    assert sample(LENS, L.Windows(starts, 2)) == -1 and b"row 1" in lib.vb_last_error() and b"windows" in lib.vb_last_error()
    t5 = torch.cat([batch["t5_cond"], batch["t5_uncond"]]).cuda()
    midi, beats = torch.zeros(B, 2 * T + 2, dtype=torch.int64, device="cuda"), torch.zeros(B, 2 * T + 2, dtype=torch.int64, device="cuda")
    arr = (C.c_int32 * B)(*LENS)
    ls = L.Lens(arr)
    rc = lib.vb_dit_precompute_cond_lens(eng.ctx.handle, L.ptr(t5), L.ptr(midi), L.ptr(beats), B, 2, T, 2 * T + 2, LC, C.byref(ls), L.ptr(cond["buf"]),
                                         L.ptr(ws), L.stream_ptr())
    assert rc == -1 and b"row 1" in lib.vb_last_error() and b"T_mel" in lib.vb_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before), "a refused call must not touch x"


# ---------------------------------------------------------------------------------------------------------------- 8
def test_cli_length_slack_files_are_byte_identical(tmp_path):
    """scripts/infer_batched.py --items_per_batch 3 --length_slack 80 over items of 200, 168 and 132 latent tokens against --items_per_batch 1:
    the same files byte for byte, from fewer sampler calls"""
    frames = [400, 336, 264]
    common = [sys.executable, os.path.join(ROOT, "scripts", "infer_batched.py"), "--synthetic", "6", "--synthetic_frames", ",".join(map(str, frames)),
              "--ddim_steps", "2", "--scales", "3", "--n_samples", "1"]
    listing = {}
    for name, extra in (("slack", ["--items_per_batch", "3", "--length_slack", "80"]), ("one", ["--items_per_batch", "1"])):
        out = tmp_path / "gen"
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
    a, b = listing["slack"], listing["one"]
    assert sorted(a) == sorted(b) and len([f for f in a if f.endswith(".wav")]) == 6
    for name in sorted(a):
        assert a[name] == b[name], f"{name} differs between --length_slack 80 and the per-item loop"
    lengths = [frames[i % 3] // harness.MEL_DOWNSAMPLE for i in range(6)]
    calls = harness.plan_row_batches(lengths, [3.0], 1, 3, length_slack=80)
    assert len(calls) == 2 and all(c["row_lengths"] == [200, 168, 132] for c in calls)
    assert len(harness.plan_row_batches(lengths, [3.0], 1, 1)) == 6
