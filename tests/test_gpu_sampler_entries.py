"""The four older sampler entry points on the GPU (vb_sample_cfg, vb_sample_cfg_keep, vb_sample_cfg_rows, vb_sample_cfg_windows, through
the C ABI): each is a one-line forward to vb_sample_cfg_sched, the only entry the Python engine calls.  A direct call of each, on the
buffers the engine itself used, gives the engine's bits and replays the engine's captured graph - the forward reaches the same
description of the call and thereby the same graph-cache entry (fixtures and argument layout: tests/test_gpu_guidance.py)."""
import ctypes as C

import pytest
import torch

from tests.helpers import SEED, clip_batch, describe
from versband_amd import _lib as L
from versband_amd import model as vm
from versband_amd import synth

pytestmark = pytest.mark.gpu
SIGMA = 1e-4
B, T, LC = 2, 40, 8
STEPS = 4               # vm.euler_tables(5)
SCALE = 3.0


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Context("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(synth.dit_shapes(synth.DiTConfig()), SEED)


@pytest.fixture(scope="module")
def base(ctx, sd):
    from versband_amd.engine import DiTEngine
    return DiTEngine(ctx, synth.DiTConfig(), sd, precision="bf16")


@pytest.fixture(scope="module")
def inp():
    return clip_batch(B, T, LC)


def _options(entry):
    """the engine's keywords for the option an entry point introduced, and that option's blocks for the direct call, over the same device
    buffers (conforming device tensors are passed to the library as they are: their addresses are in the graph key)"""
    gen = torch.Generator().manual_seed(SEED + 11)
    cin = synth.DiTConfig().in_channels
    kw, keep, rows, win, held = {"scale": SCALE}, None, None, None, []
    if entry == "vb_sample_cfg_keep":
        ref, x0k = (torch.randn(B, cin, T, generator=gen).cuda() for _ in range(2))
        mask = torch.zeros(B, T)
        mask[:, :8] = 1.0
        mask, t_next = mask.cuda(), vm.euler_times(STEPS + 1)
        tn = torch.tensor(t_next, dtype=torch.float32, device="cuda")
        kw["keep"] = (ref, x0k, mask, t_next, SIGMA)
        keep = L.Keep(ref.data_ptr(), x0k.data_ptr(), mask.data_ptr(), tn.data_ptr(), SIGMA)
        held = [ref, x0k, mask, tn]
    elif entry == "vb_sample_cfg_rows":
        scales = torch.tensor([1.5, 4.5], dtype=torch.float32, device="cuda")
        clips = torch.tensor([7, 3], dtype=torch.int64, device="cuda")
        kw.update(scale=scales, clip_ids=clips)
        rows = L.Rows(scales.data_ptr(), clips.data_ptr())
        held = [scales, clips]
    elif entry == "vb_sample_cfg_windows":
        kw["windows"] = [0, 24]               # two windows of one clip, 16 tokens of overlap
        arr = (C.c_int32 * 2)(0, 24)
        win = L.Windows(arr, 2)
        held = [arr]
    return kw, keep, rows, win, held


@pytest.mark.parametrize("entry", ["vb_sample_cfg", "vb_sample_cfg_keep", "vb_sample_cfg_rows", "vb_sample_cfg_windows"])
def test_older_entry_is_the_engines_call(ctx, sd, base, inp, entry):
    """two engine calls with the option (the second captures), then the older entry point itself on the engine's state buffer"""
    from versband_amd.engine import DiTEngine
    eng = DiTEngine(ctx, synth.DiTConfig(), sd, precision="bf16", share=base)      # its own context: its own graph cache
    idx, dts = vm.euler_tables(STEPS + 1)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).cuda()
    midi, beats, x0 = inp["midi"].cuda(), inp["beats"].cuda(), inp["x_latent"].cuda()
    kw, keep, rows, win, held = _options(entry)
    scale = kw.pop("scale")
    ref = lambda s: C.byref(s) if s is not None else None
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
        got = [eng.sample_cfg(x0, cond, idx, dts, scale, seed=5, **kw) for _ in range(2)]
        stream.synchronize()
        assert eng.graphs() == 1
        x = eng._xbuf[tuple(x0.shape)]          # the address the engine's graph was keyed with
        tt, dd = torch.tensor(idx, dtype=torch.int64, device="cuda"), torch.tensor(dts, dtype=torch.float32, device="cuda")
        ns = L.Noise(None, None, None, 5, 0, 0)
        head = (eng.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, 2, T, LC, STEPS, L.ptr(tt), L.ptr(dd), SCALE)
        tail = (C.byref(ns), None, L.ptr(eng._workspace(B, 2, T, LC)), L.stream_ptr())
        blocks = {"vb_sample_cfg": (), "vb_sample_cfg_keep": (ref(keep),), "vb_sample_cfg_rows": (ref(rows), ref(keep)),
                  "vb_sample_cfg_windows": (ref(win), ref(rows), ref(keep))}[entry]
        direct = []
        for _ in range(2):      # (twice: a call under another key would run eagerly the first time and capture a second graph now)
            x.copy_(x0)
            rc = getattr(eng.ctx.lib, entry)(*head, *blocks, *tail)
            stream.synchronize()
            assert rc == 0, eng.ctx.lib.vb_last_error()
            assert eng.graphs() == 1, f"{entry} must replay the graph of the engine's call"
            direct.append(x.clone())
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], got[1])
    for xd in direct:
        assert torch.equal(xd, got[0]), describe(f"{entry} called directly vs the engine's call", xd, got[0])
