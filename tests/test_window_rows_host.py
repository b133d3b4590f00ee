"""Host side of window rows (vb_sample_cfg_window_rows, vb_window_rows_blend): joint windows of long clips of different lengths as rows
of one sampler call.  The declarations and their binding, plan_window_rows, the planning of sample_long(lengths=, mode="joint") and the
host mirror of the library's validation, with the row named.  No GPU."""
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

# the mixed plan of tests/test_gpu_window_rows.py, clip by clip: (start, len) of every row at T = 40
GROUPS = {"A": [(0, 40), (32, 40), (60, 40)], "B": [(0, 40), (30, 40)], "C": [(0, 25)], "D": [(0, 40), (32, 17)], "E": [(0, 40), (32, 16), (40, 16)]}


def test_new_entry_points_are_declared_bound_and_additive():
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("vb_sample_cfg_window_rows", "vb_window_rows_blend"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(args.split(",")) == len(L.PROTOTYPES[name][1]), name
    blk = re.search(r"typedef struct \{([^}]*)\} vb_window_rows;", code).group(1)
    assert re.findall(r"const int32_t\*\s+([a-z0-9_]+)\s*;", blk) == [f[0] for f in L.WindowRows._fields_] == ["group", "start"]
    assert [f[1] for f in L.WindowRows._fields_] == [C.POINTER(C.c_int32)] * 2
    lens, wr = L.PROTOTYPES["vb_sample_cfg_lens"][1], L.PROTOTYPES["vb_sample_cfg_window_rows"][1]
    assert len(wr) == len(lens) + 1 and wr[:11] == lens[:11] and wr[12:] == lens[11:] and wr[11] == C.POINTER(L.WindowRows)
    lib = L.load()
    assert hasattr(lib, "vb_sample_cfg_window_rows") and hasattr(lib, "vb_window_rows_blend") and lib.vb_abi_version() == 3
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_window_rows;", src, flags=re.S).group(1)
    for needle in ("fmaf(g, x[ib] - x[ia], x[ia])", "(float)(u + 1) / (float)(ov + 1)", "start[ra] + len[ra] - start[rb]", "traj copy", "B > 64",
                   "neither read nor written", "a token under three rows", "ov > len[rb]"):
        assert needle in doc, needle


def test_the_library_refuses_a_malformed_plan_on_the_host():
    """vb_window_rows_blend validates before it launches: a malformed plan comes back as VB_E_INVALID without a GPU, and without x
    being touched (a host pointer would fault if it were)"""
    lib = L.load()
    x = np.zeros((3, 2, 40), dtype=np.float32)
    px = x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    for group, start, ln, pat in (((0, 0, 0), (0, 32, 73), None, "row 2"), ((0, 0, 0), (0, 32, 39), None, "row 2"), ((0, 1, 0), (0, 0, -1), None, "row 2"),
                                  ((0, 0, 1), (5, 5, 0), None, "row 1"), ((0, 0, 1), (0, 32, 0), (40, 7, 40), "row 1")):
        rc = lib.vb_window_rows_blend(px, i32(group), i32(start), i32(ln) if ln else None, 3, 2, 40, None)
        assert rc == -1 and pat in lib.vb_last_error().decode(), (group, start, lib.vb_last_error())
    assert lib.vb_window_rows_blend(px, None, i32((0, 1, 2)), None, 3, 2, 40, None) == -1 and b"group" in lib.vb_last_error()
    assert lib.vb_window_rows_blend(px, i32((0, 1, 2)), None, None, 3, 2, 40, None) == -1 and b"start" in lib.vb_last_error()
    assert lib.vb_window_rows_blend(px, i32([0] * 65), i32(list(range(65))), None, 65, 2, 40, None) == -1 and b"row 64" in lib.vb_last_error()
    # no group with two rows: nothing to launch, nothing touched
    assert lib.vb_window_rows_blend(px, i32((0, 1, 2)), i32((0, 0, 7)), None, 3, 2, 40, None) == 0
    assert not x.any()


def test_plan_window_rows_reproduces_plan_windows_and_covers_every_clip_once():
    for lengths, window, overlap in (([100, 70, 25, 40, 41, 49], 40, 8), ([1800, 2200, 2600, 3000], 1500, 128)):
        group, start, row_len = longform.plan_window_rows(lengths, window, overlap)
        assert len(group) == len(start) == len(row_len)
        assert group == sorted(group), "clip by clip"
        for b, T_b in enumerate(lengths):
            rows = [r for r, g in enumerate(group) if g == b]
            plan = [(start[r], row_len[r]) for r in rows]
            assert plan == longform.plan_windows(T_b, window, overlap)
            if T_b <= window:
                assert plan == [(0, T_b)]
            cover = np.zeros(T_b, dtype=np.int64)
            for s, m, known in longform.plan_continue(plan):
                cover[s + known:s + m] += 1
            assert (cover == 1).all(), f"clip {b} of {T_b} tokens"
    group, _, row_len = longform.plan_window_rows([1800, 2200, 2600, 3000], 1500, 128)
    assert [group.count(b) for b in range(4)] == [2, 2, 2, 3] and row_len == [1500] * 9


def _mixed_rows():
    """the five groups' rows interleaved: A0 B0 A1 C0 B1 D0 E0 A2 D1 E1 E2"""
    order = [("A", 0), ("B", 0), ("A", 1), ("C", 0), ("B", 1), ("D", 0), ("E", 0), ("A", 2), ("D", 1), ("E", 1), ("E", 2)]
    group = [ord(g) - ord("A") for g, _ in order]
    start = [GROUPS[g][w][0] for g, w in order]
    lens = [GROUPS[g][w][1] for g, w in order]
    return group, start, lens


def test_engine_validates_the_row_plan_with_the_row_named():
    from versband_amd.engine import DiTEngine
    T = 40
    group, start, lens = _mixed_rows()
    ws, held, pairs = DiTEngine._window_rows_struct((group, start), 11, T, lens)
    assert [ws.group[i] for i in range(11)] == group and [ws.start[i] for i in range(11)] == start and list(held[1]) == start
    # {ra, rb, off_a, ov}: A 0-2 (8), 2-7 (12); B 1-4 (10); D 5-8 (8); E 6-9 (8), 9-10 (8 of the middle row's 16)
    assert pairs == [(0, 2, 32, 8), (1, 4, 30, 10), (2, 7, 28, 12), (5, 8, 32, 8), (6, 9, 32, 8), (9, 10, 8, 8)]
    assert DiTEngine._window_rows_struct((torch.tensor([0, 1, 0]), np.array([0, 0, 40])), 3, T)[2] == [], "rows that only touch have no pair"
    assert DiTEngine._window_rows_struct(([3, 9], [0, 5]), 2, T)[2] == [], "groups of one row"
    bad = [(([0, 0, 0], [0, 32, 73]), None, ValueError, r"gap between row 1 .* and row 2"),
           (([0, 1, 0], [0, 0, 41]), None, ValueError, r"gap between row 0 .* and row 2"),
           (([0, 0], [32, 0]), None, ValueError, r"row 1 at 0 does not come after row 0"),
           (([0, 0], [5, 5]), None, ValueError, r"row 1 at 5 does not come after row 0"),
           (([0, 0, 0], [0, 32, 39]), None, ValueError, r"row 2 at 39 reaches into row 0 .* three rows"),
           (([0, 1, 0, 0], [0, 0, 32, 36]), [40, 40, 17, 40], ValueError, r"row 3 at 36 reaches into row 0 .* three rows"),
           (([0, 0], [0, 32]), [40, 7], ValueError, r"row 1 of length 7 lies inside its overlap of 8"),
           (([0, 0], [0, 26]), [25, 40], ValueError, r"gap between row 0 at 0 \(length 25\) and row 1"),
           (([0, 1, 0], [0, -1, 32]), None, ValueError, r"start\[1\] = -1"),
           (([0, 0], [0, 32, 60]), None, ValueError, r"start has 3 entries for 2 rows"),
           (([0.0, 0.0], [0, 32]), None, TypeError, "integers"),
           ((None, [0, 32]), None, ValueError, "group and start"),
           (([0, 0], None), None, ValueError, "group and start"),
           (7, None, TypeError, r"pair \(group, start\)")]
    for wr, ln, exc, pat in bad:
        B = len(wr[0]) if isinstance(wr, tuple) and wr[0] is not None else 2
        with pytest.raises(exc, match=pat):
            DiTEngine._window_rows_struct(wr, B, T, ln)
    with pytest.raises(ValueError, match="65 rows .* row 64"):
        DiTEngine._window_rows_struct(([0] * 65, list(range(65))), 65, T)
    with pytest.raises(ValueError, match="window_rows and windows do not go together"):
        DiTEngine._window_rows_struct(([0, 0], [0, 32]), 2, T, None, windows=[0, 32])
    DiTEngine._window_rows_struct(([0, 0], [0, 32]), 2, T, None, windows=[0])
    # the refusal of windows beside lengths stays word for word
    with pytest.raises(ValueError, match="lengths and joint windows do not go together: windows are equal-length by construction"):
        DiTEngine._lens_struct([40, 25], 2, T, windows=[0, 32])


class _RowsEngine:
    """records what sample_long hands to the sampler; a row's "result" is its start noise plus one, so rows cut from one start noise
    agree in their overlaps as the real joint call's rows do"""

    def __init__(self, max_len):
        self.cfg = SimpleNamespace(max_len=max_len)
        self.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None)
        self.calls = []

    def precompute_cond(self, t5, midi, beats, T, persistent=False, **kw):
        assert midi.shape[1] == beats.shape[1] == 2 * T and persistent
        return {"T": T, "midi": midi.clone(), "beats": beats.clone(), "t5": t5.clone(), "kw": dict(kw)}

    def sample_cfg(self, x, cond, t_idx_table, dt_table, scale, seed=0, clip_base=0, **kw):
        assert x.shape[2] == cond["T"]
        self.calls.append(dict(x=x.clone(), clip_base=clip_base, seed=seed, cond=cond, scale=scale, kw=dict(kw)))
        return x + 1.0


def _inputs(B, T):
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(B, 20, T, generator=g)
    midi = (torch.arange(2 * T).repeat(B, 1) + 1000 * torch.arange(B).unsqueeze(1)).unsqueeze(1)
    t5 = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1).expand(B, 4, 8).contiguous()
    return x0, midi, midi % 3, t5


def test_sample_long_with_lengths_is_one_call_of_every_clips_windows():
    B, T, window, overlap, lengths = 3, 100, 40, 8, [100, 70, 25]
    x0, midi, beats, t5 = _inputs(B, T)
    idx, dts = vm.euler_tables(4)
    eng = _RowsEngine(window)
    z, parts = longform.sample_long(eng, x0, t5, t5 + 10, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5,
                                    mode="joint", return_windows=True, lengths=lengths)
    assert len(eng.calls) == 1
    call = eng.calls[0]
    group, start, row_len = [0, 0, 0, 1, 1, 2], [0, 32, 60, 0, 30, 0], [40, 40, 40, 40, 40, 25]
    assert (group, start, row_len) == longform.plan_window_rows(lengths, window, overlap)
    # clip b's window w under the key of sample_long on that clip alone with clip_base + b: (clip_base + b) * nw_b + w
    assert call["kw"] == {"clip_ids": [15, 16, 17, 12, 13, 7], "window_rows": (group, start), "lengths": row_len, "guidance": None}
    assert call["cond"]["kw"] == {"lengths": row_len} and call["clip_base"] == 0 and call["seed"] == 3
    assert call["x"].shape == (6, 20, 40)
    for r, (b, s, m) in enumerate(zip(group, start, row_len)):
        assert torch.equal(call["x"][r, :, :m], x0[b, :, s:s + m]) and not call["x"][r, :, m:].any()
        assert torch.equal(call["cond"]["midi"][r, :2 * m], midi[b, 0, 2 * s:2 * (s + m)])
        assert torch.equal(call["cond"]["beats"][r, :2 * m], beats[b, 0, 2 * s:2 * (s + m)])
        assert float(call["cond"]["t5"][r, 0, 0]) == b and float(call["cond"]["t5"][6 + r, 0, 0]) == b + 10
    want = torch.zeros_like(x0)
    for b, T_b in enumerate(lengths):
        want[b, :, :T_b] = x0[b, :, :T_b] + 1.0
        assert [tuple(p.shape) for p in parts[b]] == [(1, 20, m) for _, m in longform.plan_windows(T_b, window, overlap)]
        for (s, m), p in zip(longform.plan_windows(T_b, window, overlap), parts[b]):
            assert torch.equal(p, z[b:b + 1, :, s:s + m])
    assert torch.equal(z, want), "every token from exactly one window, zeros behind each clip's end"
    # the keys are those of the per-clip calls
    for b, T_b in enumerate(lengths):
        one = _RowsEngine(window)
        longform.sample_long(one, x0[b:b + 1, :, :T_b], t5[b:b + 1], t5[b:b + 1], midi[b:b + 1, :, :2 * T_b], beats[b:b + 1, :, :2 * T_b], idx,
                             dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5 + b, mode="joint")
        nw = group.count(b)
        assert [one.calls[0]["clip_base"] + w for w in range(nw)] == [k for k, g in zip(call["kw"]["clip_ids"], group) if g == b]


def test_lengths_belong_to_joint_mode_and_equal_lengths_are_todays_call():
    B, T, window, overlap = 2, 100, 40, 8
    x0, midi, beats, t5 = _inputs(B, T)
    idx, dts = vm.euler_tables(4)
    for mode in ("crossfade", "continue"):
        with pytest.raises(ValueError, match='lengths belong to mode="joint"'):
            longform.sample_long(_RowsEngine(window), x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, mode=mode,
                                 lengths=[100, 70], t_next=vm.euler_times(4))
    for bad, pat in (([100], "1 entries for 2 clips"), ([100, 0], r"lengths\[1\] = 0"), ([101, 70], r"lengths\[0\] = 101")):
        with pytest.raises(ValueError, match=pat):
            longform.sample_long(_RowsEngine(window), x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, mode="joint", lengths=bad)
    with pytest.raises(ValueError, match="exactly 2 x 100 frames"):
        longform.sample_long(_RowsEngine(window), x0, t5, t5, midi[:, :, :198], beats[:, :, :198], idx, dts, 3.0, window=window, overlap=overlap,
                             mode="joint", lengths=[100, 70])
    # all lengths equal to T: the windows= call of today, argument for argument
    a, b = _RowsEngine(window), _RowsEngine(window)
    za = longform.sample_long(a, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5, mode="joint")
    zb = longform.sample_long(b, x0, t5, t5, midi, beats, idx, dts, 3.0, window=window, overlap=overlap, seed=3, clip_base=5, mode="joint",
                              lengths=torch.tensor([100, 100]))
    assert torch.equal(za, zb) and len(a.calls) == len(b.calls) == 1
    ca, cb = a.calls[0], b.calls[0]
    assert ca["kw"] == cb["kw"] == {"windows": [0, 32, 60]} and ca["cond"]["kw"] == cb["cond"]["kw"] == {} and ca["clip_base"] == cb["clip_base"]
    assert torch.equal(ca["x"], cb["x"]) and torch.equal(ca["cond"]["midi"], cb["cond"]["midi"])
    # ... and the same rows as the window-rows plan of equal lengths, which is the interleaved layout read clip by clip
    group, start, row_len = longform.plan_window_rows([100, 100], window, overlap)
    assert row_len == [40] * 6
    for r, (g, s) in enumerate(zip(group, start)):
        w = [0, 32, 60].index(s)
        assert torch.equal(ca["x"][w * B + g], x0[g, :, s:s + 40])
