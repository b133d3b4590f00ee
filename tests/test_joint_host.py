"""Host side of joint window sampling (vb_sample_cfg_windows, vb_window_blend): the declarations and their binding, the planning of
sample_long(mode="joint") and the validation of a window plan.  No GPU."""
import ctypes as C
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


def test_new_entry_points_are_declared_bound_and_additive():
    """both functions and vb_windows sit in the header and in the binding, field for field; the ABI version did not move; the header states
    the formula and the weight where an integrator reads them"""
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("vb_sample_cfg_windows", "vb_window_blend"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in L.PROTOTYPES, name
    blk = re.search(r"typedef struct \{([^}]*)\} vb_windows;", code).group(1)
    fields = re.findall(r"(const int32_t\*|int)\s+([a-z0-9_]+)\s*;", blk)
    assert [n for _, n in fields] == [f[0] for f in L.Windows._fields_] == ["starts", "nw"]
    assert [C.POINTER(C.c_int32) if t.endswith("*") else L.c_int for t, _ in fields] == [f[1] for f in L.Windows._fields_]
    rows, win = L.PROTOTYPES["vb_sample_cfg_rows"][1], L.PROTOTYPES["vb_sample_cfg_windows"][1]
    assert len(win) == len(rows) + 1 and win[:11] == rows[:11] and win[12:] == rows[11:]      # the window block goes in before the rows block
    assert win[11] == C.POINTER(L.Windows)
    assert L.PROTOTYPES["vb_window_blend"] == (L.c_int, [L.c_void_p, C.POINTER(C.c_int32), L.c_int, L.c_int, L.c_int, L.c_int, L.c_void_p])
    # the argument lists of the header, by count
    for name in ("vb_sample_cfg_windows", "vb_window_blend"):
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(args.split(",")) == len(L.PROTOTYPES[name][1]), name
    lib = L.load()
    assert hasattr(lib, "vb_sample_cfg_windows") and hasattr(lib, "vb_window_blend") and lib.vb_abi_version() == 3
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_windows;", src, flags=re.S).group(1)
    for needle in ("fmaf(g, x[ib] - x[ia], x[ia])", "(u + 1) / (ov + 1)", "[nw*Bc][C][n]", "w*Bc + b", "bit-identical after every step",
                   "traj copy", "B % nw != 0", "starts[w+2] < starts[w] + n"):
        assert needle in doc, needle


class _JointEngine:
    """records what sample_long hands to the sampler; accepts windows=.  A row's "result" is its start noise plus one, so rows cut from one
    start noise agree in their overlaps as the real joint call's rows do."""

    def __init__(self, max_len):
        self.cfg = SimpleNamespace(max_len=max_len)
        self.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None)
        self.calls = []

    def precompute_cond(self, t5, midi, beats, T, persistent=False):
        assert midi.shape[1] == beats.shape[1] == 2 * T and persistent
        return {"T": T, "midi": midi.clone(), "beats": beats.clone(), "t5_rows": t5.shape[0]}

    def sample_cfg(self, x, cond, t_idx_table, dt_table, scale, seed=0, clip_base=0, **kw):
        assert x.shape[2] == cond["T"]
        self.calls.append(dict(x=x.clone(), clip_base=clip_base, seed=seed, midi=cond["midi"], beats=cond["beats"], t5_rows=cond["t5_rows"],
                               scale=scale, kw=dict(kw)))
        return x + 1.0


def _inputs(B, T):
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, 20, T, generator=g)
    midi = (torch.arange(2 * T).repeat(B, 1) + 1000 * torch.arange(B).unsqueeze(1)).unsqueeze(1)
    return x0, midi, midi % 3, torch.zeros(B, 4, 8)


def test_joint_mode_is_one_call_of_the_crossfade_rows_with_the_window_starts():
    B, T, window, overlap = 2, 100, 40, 8
    x0, midi, beats, t5 = _inputs(B, T)
    idx, dts = vm.euler_tables(4)
    eng = _JointEngine(window)
    z, parts = longform.sample_long(eng, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5,
                                    mode="joint", return_windows=True)
    plan = longform.plan_windows(T, window, overlap)
    assert [s for s, _ in plan] == [0, 32, 60]
    nw, n = len(plan), window
    assert len(eng.calls) == 1
    call = eng.calls[0]
    assert call["kw"] == {"windows": [0, 32, 60]}
    assert call["clip_base"] == 5 * nw and call["seed"] == 3 and call["scale"] == 3.0
    assert call["x"].shape == (nw * B, 20, n) and call["t5_rows"] == 2 * nw * B
    for w, (s, _) in enumerate(plan):          # row = w * B + b, as in cross-fade mode
        assert torch.equal(call["x"][w * B:(w + 1) * B], x0[:, :, s:s + n])
        assert torch.equal(call["midi"][w * B:(w + 1) * B], midi[:, 0, 2 * s:2 * (s + n)])
        assert torch.equal(call["beats"][w * B:(w + 1) * B], beats[:, 0, 2 * s:2 * (s + n)])
        assert torch.equal(parts[w], x0[:, :, s:s + n] + 1.0)
    # the cross-fade call of the same arguments: the same rows, conditioning and noise key, no windows keyword
    eng2 = _JointEngine(window)
    longform.sample_long(eng2, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5)
    assert len(eng2.calls) == 1 and eng2.calls[0]["kw"] == {}, "the default mode must not pass a windows keyword"
    for k in ("x", "midi", "beats"):
        assert torch.equal(eng2.calls[0][k], call[k]), k
    assert (eng2.calls[0]["clip_base"], eng2.calls[0]["seed"], eng2.calls[0]["t5_rows"]) == (call["clip_base"], call["seed"], call["t5_rows"])
    # the stitch: plan_continue's spans, every token from exactly one window
    cover = np.zeros(T, dtype=np.int64)
    want = torch.full_like(x0, float("nan"))
    for (s, m, known), p in zip(longform.plan_continue(plan), parts):
        cover[s + known:s + m] += 1
        want[:, :, s + known:s + m] = p[:, :, known:]
    assert (cover == 1).all()
    assert torch.equal(z, want) and torch.equal(z, x0 + 1.0)
    # without return_windows: the stitched tensor alone
    z2 = longform.sample_long(_JointEngine(window), x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3,
                              clip_base=5, mode="joint")
    assert torch.equal(z2, z)


def test_joint_mode_of_a_short_clip_is_the_plain_call():
    B, T = 2, 40
    x0, midi, beats, t5 = _inputs(B, T)
    idx, dts = vm.euler_tables(4)
    eng = _JointEngine(40)
    z = longform.sample_long(eng, x0, t5, t5, midi, beats, idx, dts, 3.0, window=40, overlap=8, seed=3, clip_base=5, mode="joint")
    assert len(eng.calls) == 1 and eng.calls[0]["kw"] == {} and eng.calls[0]["clip_base"] == 5 and eng.calls[0]["x"].shape == (B, 20, T)
    assert torch.equal(z, x0 + 1.0)
    z, parts = longform.sample_long(_JointEngine(40), x0, t5, t5, midi, beats, idx, dts, 3.0, window=40, overlap=8, mode="joint",
                                    return_windows=True)
    assert len(parts) == 1 and torch.equal(parts[0], z)


def test_modes_and_return_windows():
    x = torch.zeros(1, 20, 100)
    with pytest.raises(ValueError, match=r"crossfade \| continue \| joint"):
        longform.sample_long(None, x, None, None, None, None, [0], [1.0], 3.0, mode="blend")
    x0, midi, beats, t5 = _inputs(1, 100)
    with pytest.raises(ValueError, match="return_windows"):
        longform.sample_long(_JointEngine(40), x0, t5, t5, midi, beats, [0], [1.0], 3.0, window=40, overlap=8, return_windows=True)


def test_engine_validates_the_window_plan():
    """DiTEngine.sample_cfg(windows=...) checks the plan on the host, with the window named, before anything is launched"""
    from versband_amd.engine import DiTEngine
    B, T = 6, 40
    ws, arr = DiTEngine._windows_struct([0, 32, 60], B, T)
    assert ws.nw == 3 and [ws.starts[i] for i in range(3)] == [0, 32, 60] and list(arr) == [0, 32, 60]
    for ok in ([0], [0, 40, 80], (0, 30, 60), torch.tensor([0, 32, 60]), np.array([0, 1, 40])):
        DiTEngine._windows_struct(ok, B, T)
    bad = [([0, 32, 73], ValueError, "gap"),
           ([0, 41], ValueError, "gap"),
           ([32, 0], ValueError, "descending"),
           ([0, 40, 40], ValueError, "descending"),
           ([0, 32, 39], ValueError, "three windows"),
           ([0, 10, 20], ValueError, "three windows"),
           ([-1, 32, 60], ValueError, "window 0"),
           ([0, 30, 60, 90], ValueError, "B % nw"),
           ([], ValueError, "0 windows"),
           (list(range(0, 65 * 40, 40)), ValueError, "65 windows"),
           ([0.0, 32.0], TypeError, "integers"),
           (7, TypeError, "sequence")]
    for starts, exc, pat in bad:
        with pytest.raises(exc, match=pat):
            DiTEngine._windows_struct(starts, B, T)
    with pytest.raises(ValueError, match="B % nw"):
        DiTEngine._windows_struct([0, 32, 60], 4, T)
