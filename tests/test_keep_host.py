"""Host side of the known-region sampler (vb_sample_cfg_keep): the time table, argument validation, the planning of
sample_long(mode="continue") and the binding of the new entry point.  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from versband_amd import _lib as L
from versband_amd import longform
from versband_amd import model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("timesteps,t_start", [(4, None), (25, None), (50, None), (51, None), (25, 3), (51, 17), (5, 1), (6, 2)])
def test_euler_times_is_the_float32_time_after_each_step(timesteps, t_start):
    """restated in numpy float32: t_span = linspace(0, 1, n)[t_start:], dt = t_span[k + 1] - t, t += dt; the index table of euler_tables is
    trunc(t * 1000) of the time BEFORE each step, i.e. of [t_0] + euler_times[:-1]"""
    idx, dts = vm.euler_tables(timesteps, t_start)
    times = vm.euler_times(timesteps, t_start)
    span = torch.linspace(0, 1, timesteps).numpy().astype(np.float32)
    if t_start is not None:
        span = span[t_start:]
    assert len(times) == len(idx) == len(dts) == len(span) - 1
    t = np.float32(span[0])
    for k in range(len(span) - 1):
        assert idx[k] == int(np.float32(t * np.float32(1000))), (k, idx[k], t)
        dt = np.float32(span[k + 1] - t)
        assert np.float32(dts[k]) == dt
        t = np.float32(t + dt)
        assert np.float32(times[k]) == t and isinstance(times[k], float), (k, times[k], t)
    assert times[-1] == 1.0          # the path ends at t = 1: a kept token ends at ref + sigma_min * x0
    # what the library's entry projection relies on: t_0 = t_next[0] - dt[0] exactly
    assert np.float32(np.float32(times[0]) - np.float32(dts[0])) == np.float32(span[0])


def _sampler():
    model = SimpleNamespace(num_timesteps=1000, sigma_min=1e-4, device=torch.device("cpu"), channels=0, mel_dim=20, mel_length=16)
    return vm.CFMSampler(model, 1000)


def test_sampler_refuses_a_known_region_without_its_noise_when_t_start_is_set():
    s = _sampler()
    x = torch.zeros(2, 20, 16)
    with pytest.raises(ValueError, match="keep_noise"):
        s.sample_cfg({}, 3.0, {}, batch_size=2, timesteps=5, shape=(20, 16), x_latent=x, t_start=2, x_known=x, keep_mask=torch.ones(16))
    with pytest.raises(ValueError, match="keep_noise"):
        s.sample({}, batch_size=2, timesteps=5, shape=(20, 16), x_latent=x, t_start=2, x_known=x, keep_mask=torch.ones(2, 16))
    with pytest.raises(ValueError, match="go together"):
        s.sample_cfg({}, 3.0, {}, batch_size=2, timesteps=5, shape=(20, 16), x_latent=x, x_known=x)
    with pytest.raises(ValueError, match="go together"):
        s.sample_cfg({}, 3.0, {}, batch_size=2, timesteps=5, shape=(20, 16), x_latent=x, keep_mask=torch.ones(16))


def test_keep_block_validates_and_broadcasts():
    shape = (2, 20, 16)
    x = torch.randn(shape)
    z = torch.randn(shape)
    ref, x0, mask, t_next, sigma = vm.keep_block(z, torch.ones(16), None, x, None, shape, 5, 1e-4)
    assert ref is not None and x0.data_ptr() == x.data_ptr() and tuple(mask.shape) == (2, 16) and mask.is_contiguous()
    assert t_next == vm.euler_times(5) and sigma == pytest.approx(1e-4)
    assert vm.keep_block(None, None, None, x, None, shape, 5, 1e-4) is None
    *_, t_next = vm.keep_block(z, torch.ones(2, 16), x, x, 2, shape, 5, 1e-4)[:4]
    assert t_next == vm.euler_times(5, 2)
    for bad in (torch.full((16,), 1.5), torch.full((16,), -0.1), torch.full((16,), float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            vm.keep_block(z, bad, None, x, None, shape, 5, 1e-4)
    with pytest.raises(ValueError, match="keep_mask has shape"):
        vm.keep_block(z, torch.ones(3, 16), None, x, None, shape, 5, 1e-4)
    with pytest.raises(ValueError, match="keep_mask has shape"):
        vm.keep_block(z, torch.ones(15), None, x, None, shape, 5, 1e-4)
    with pytest.raises(ValueError, match="x_known has shape"):
        vm.keep_block(z[:, :, :8], torch.ones(16), None, x, None, shape, 5, 1e-4)
    with pytest.raises(ValueError, match="keep_noise has shape"):
        vm.keep_block(z, torch.ones(16), x[:1], x, None, shape, 5, 1e-4)
    with pytest.raises(ValueError, match="without"):
        vm.keep_block(None, None, x, x, None, shape, 5, 1e-4)


def test_engine_validates_the_keep_block():
    """DiTEngine.sample_cfg(keep=...) checks shapes, dtypes, devices, the mask range and the table length before anything is launched
    (the method needs the engine's device, channel count and table cache only, so a stand-in serves without a GPU)"""
    from versband_amd.engine import DiTEngine
    eng = SimpleNamespace(ctx=SimpleNamespace(device=torch.device("cpu")), cfg=SimpleNamespace(in_channels=20), _tables={})
    B, T, n = 2, 16, 4
    z, x, m, tn = torch.randn(B, 20, T), torch.randn(B, 20, T), torch.ones(B, T), vm.euler_times(n + 1)
    ks, held = DiTEngine._keep_struct(eng, (z, x, m, tn, 1e-4), B, T, n)
    assert ks.ref == z.data_ptr() and ks.x0 == x.data_ptr() and ks.mask == m.data_ptr() and ks.sigma_min == pytest.approx(1e-4)
    assert held[3].dtype == torch.float32 and held[3].tolist() == [float(np.float32(v)) for v in tn] and ks.t_next == held[3].data_ptr()
    ks2, _ = DiTEngine._keep_struct(eng, dict(ref=z, x0=x, mask=m, t_next=tn, sigma_min=1e-4), B, T, n)
    assert (ks2.ref, ks2.x0, ks2.mask, ks2.t_next) == (ks.ref, ks.x0, ks.mask, ks.t_next)
    bad = [((z[:, :, :8], x, m, tn, 1e-4), ValueError, "ref has shape"),
           ((z, x[:1], m, tn, 1e-4), ValueError, "x0 has shape"),
           ((z, x, m[0], tn, 1e-4), ValueError, "mask has shape"),
           ((z.double(), x, m, tn, 1e-4), TypeError, "float32"),
           ((z, x, m.bool(), tn, 1e-4), TypeError, "float32"),
           ((z, x, m * 1.01, tn, 1e-4), ValueError, r"\[0, 1\]"),
           ((z, x, m - 1.5, tn, 1e-4), ValueError, r"\[0, 1\]"),
           ((z, x, m, tn[:-1], 1e-4), ValueError, "t_next has"),
           ((z, x, m, tn), ValueError, "expected"),
           (dict(ref=z, x0=x, mask=m, t_next=tn), ValueError, "keys"),
           ((z.numpy(), x, m, tn, 1e-4), TypeError, "tensor")]
    for blk, exc, pat in bad:
        with pytest.raises(exc, match=pat):
            DiTEngine._keep_struct(eng, blk, B, T, n)
    if not torch.cuda.is_available():
        meta = torch.empty(B, 20, T, device="meta")
        with pytest.raises(ValueError, match="lives on"):
            DiTEngine._keep_struct(eng, (meta, x, m, tn, 1e-4), B, T, n)


@pytest.mark.parametrize("T,window,overlap,known", [
    (4500, 1500, 128, [0, 128, 128, 1244]),       # configs[4]: windows at 0 / 1372 / 2744 / 3000 - the last one reaches back 4244 - 3000 tokens
    (3100, 1500, 128, [0, 128, 1272]),            # ragged
    (100, 40, 8, [0, 8, 12]),                     # windows at 0 / 32 / 60
    (80, 48, 16, [0, 16]),
    (1500, 1500, 128, [0]),                       # one window: nothing to hold
])
def test_continue_mode_plan_holds_each_whole_overlap_and_covers_the_clip_once(T, window, overlap, known):
    plan = longform.plan_windows(T, window, overlap)
    cont = longform.plan_continue(plan)
    assert [(s, n) for s, n, _ in cont] == plan
    assert [k for _, _, k in cont] == known
    cover = np.zeros(T, dtype=np.int64)
    for w, (s, n, k) in enumerate(cont):
        assert 0 <= k < n
        if w:
            ps, pn = plan[w - 1]
            assert k == ps + pn - s          # the whole overlap with the previous window
            assert s + k <= T
        cover[s + k:s + n] += 1
    assert (cover == 1).all(), "the stitch must cover [0, T) exactly once"


def test_sample_long_rejects_unknown_modes_before_touching_the_engine():
    x = torch.zeros(1, 20, 100)
    with pytest.raises(ValueError, match="mode"):
        longform.sample_long(None, x, None, None, None, None, [0], [1.0], 3.0, mode="blend")


def test_new_entry_point_is_declared_bound_and_additive():
    """vb_sample_cfg_keep sits in the header and in PROTOTYPES (tests/test_abi.py:test_header_and_binding_agree compares the two sets),
    the vb_keep struct matches its ctypes mirror field for field, and the ABI version did not move"""
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+vb_sample_cfg_keep\s*\(", code) and "vb_sample_cfg_keep" in L.PROTOTYPES
    blk = re.search(r"typedef struct \{([^}]*)\} vb_keep;", code).group(1)
    fields = re.findall(r"(const float\*|float)\s+([a-z0-9_]+)\s*;", blk)
    assert [n for _, n in fields] == [f[0] for f in L.Keep._fields_] == ["ref", "x0", "mask", "t_next", "sigma_min"]
    assert [L.c_void_p if t.endswith("*") else L.c_float for t, _ in fields] == [f[1] for f in L.Keep._fields_]
    plain, keep = L.PROTOTYPES["vb_sample_cfg"][1], L.PROTOTYPES["vb_sample_cfg_keep"][1]
    assert len(keep) == len(plain) + 1 and keep[:11] == plain[:11] and keep[12:] == plain[11:]      # the keep block goes in before the noise block
    lib = L.load()
    assert hasattr(lib, "vb_sample_cfg_keep") and lib.vb_abi_version() == 3
    # the formula, the layouts and the end point of a kept token are stated where an integrator reads them
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_keep;", src, flags=re.S).group(1)
    for needle in ("fmaf(tn, ref, (1 - (1 - sigma_min) * tn) * x0)", "fmaf(m, r, (1 - m) * xn)", "[B][C][T]", "[B][T]", "ref + sigma_min * x0"):
        assert needle in doc, needle


class _FakeEngine:
    """records what sample_long hands to the sampler; a window's "result" is its start noise plus one, with the known tokens returned
    as a kept token ends: ref + sigma_min * x0"""

    def __init__(self, max_len):
        self.cfg = SimpleNamespace(max_len=max_len)
        self.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None)
        self.calls = []

    def precompute_cond(self, t5, midi, beats, T, persistent=False):
        assert midi.shape[1] == beats.shape[1] == 2 * T and persistent
        return {"T": T, "midi": midi.clone()}

    def sample_cfg(self, x, cond, t_idx_table, dt_table, scale, seed=0, clip_base=0, keep=None):
        assert x.shape[2] == cond["T"]
        out = x + 1.0
        rec = dict(x=x.clone(), clip_base=clip_base, seed=seed, midi=cond["midi"], keep=None)
        if keep is not None:
            ref, x0, mask, t_next, sigma = keep
            rec["keep"] = (ref.clone(), x0.clone(), mask.clone(), list(t_next), sigma)
            m = mask.unsqueeze(1)
            out = m * (ref + sigma * x0) + (1 - m) * out
        self.calls.append(rec)
        return out


@pytest.mark.parametrize("B,T,window,overlap", [(2, 100, 40, 8), (1, 4500, 1500, 128)])
def test_continue_mode_threads_each_window_through_the_previous_one(B, T, window, overlap):
    eng = _FakeEngine(window)
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, 20, T, generator=g)
    midi = torch.arange(2 * T).repeat(B, 1).unsqueeze(1)
    beats = midi % 3
    t5 = torch.zeros(B, 4, 8)
    times = vm.euler_times(4)
    idx, dts = vm.euler_tables(4)
    z, parts = longform.sample_long(eng, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5,
                                    mode="continue", t_next=times, sigma_min=1e-4, return_windows=True)
    cont = longform.plan_continue(longform.plan_windows(T, window, overlap))
    nw = len(cont)
    assert len(eng.calls) == len(parts) == nw
    want = torch.empty_like(x0)
    for w, ((s, n, known), call) in enumerate(zip(cont, eng.calls)):
        assert call["clip_base"] == 5 * nw + w * B and call["seed"] == 3        # the keys of rows [w*B, (w+1)*B) of the cross-fade batch
        assert torch.equal(call["x"], x0[:, :, s:s + n]) and torch.equal(call["midi"], midi[:, 0, 2 * s:2 * (s + n)])
        if w == 0:
            assert call["keep"] is None
            want[:, :, :n] = x0[:, :, :n] + 1.0
            continue
        ref, xk, mask, t_next, sigma = call["keep"]
        assert t_next == times and sigma == 1e-4
        assert torch.equal(xk, x0[:, :, s:s + n]), "keep_noise is the window's own slice of the start noise"
        assert torch.equal(mask[:, :known], torch.ones(B, known)) and not mask[:, known:].any()
        assert torch.equal(ref[:, :, :known], want[:, :, s:s + known]), "the known content is the previous result's tail"
        want[:, :, s + known:s + n] = x0[:, :, s + known:s + n] + 1.0
        assert torch.equal(parts[w][:, :, :known], ref[:, :, :known] + 1e-4 * xk[:, :, :known])
    assert torch.equal(z, want)
    # the default mode never passes a keep block and makes one call of nw * B rows
    eng2 = _FakeEngine(window)
    eng2.ctx.lib = None
    longform.sample_long(eng2, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5)
    assert len(eng2.calls) == 1 and eng2.calls[0]["keep"] is None and eng2.calls[0]["x"].shape[0] == nw * B and eng2.calls[0]["clip_base"] == 5 * nw
