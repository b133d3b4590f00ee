"""Host side of per-step guidance weights (vb_sample_cfg_sched): the binding of the new entry point, guidance_interval_weights on the
solver's grids, the validation in DiTEngine.sample_cfg and CFMSampler.sample_cfg, and the argument plumbing of scripts/infer_batched.py.
No GPU."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from versband_amd import _lib as L
from versband_amd import model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sched_entry_point_is_declared_bound_and_additive():
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+vb_sample_cfg_sched\s*\(", code) and "vb_sample_cfg_sched" in L.PROTOTYPES
    blk = re.search(r"typedef struct \{([^}]*)\} vb_guidance;", code).group(1)
    assert re.findall(r"const float\*\s+([a-z0-9_]+)\s*;", blk) == [f[0] for f in L.Guidance._fields_] == ["weight"]
    assert L.C.sizeof(L.Guidance) == L.C.sizeof(L.c_void_p)
    win, sched = L.PROTOTYPES["vb_sample_cfg_windows"][1], L.PROTOTYPES["vb_sample_cfg_sched"][1]
    assert len(sched) == len(win) + 1 and sched[:11] == win[:11] and sched[12:] == win[11:]      # the guidance block goes in before the windows
    lib = L.load()
    assert hasattr(lib, "vb_sample_cfg_sched") and lib.vb_abi_version() == 3
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_guidance;", src, flags=re.S).group(1)
    for needle in ("fmaf(weight[k], s - 1, 1)", "fmaf(dt, v_c, x)", "[0, 16]", "VB_E_INVALID", "n_branch == 1", "VALUES", "as if every step had two branches"):
        assert needle in doc, needle


@pytest.mark.parametrize("timesteps,lo,hi,want", [
    (4, 0.0, 1.0, [1, 1, 1]),                      # grid 0, 1/3, 2/3 (, 1): every step starts inside
    (4, 1 / 3, 2 / 3, [0, 1, 1]),                  # both ends exactly on grid points (float32 of the grid)
    (4, 0.34, 0.66, [0, 0, 0]),
    (6, 0.2, 0.6, [0, 1, 1, 1, 0]),                # grid 0, .2, .4, .6, .8: ends on grid points
    (6, 0.21, 0.79, [0, 0, 1, 1, 0]),
    (6, 0.0, 0.0, [1, 0, 0, 0, 0]),
    (6, 0.9, 1.0, [0, 0, 0, 0, 0]),                # the last step starts at 0.8
])
def test_interval_weights_on_the_solver_grid(timesteps, lo, hi, want):
    grid = torch.linspace(0, 1, timesteps)
    lo = float(grid[round(lo * (timesteps - 1))]) if abs(lo * (timesteps - 1) - round(lo * (timesteps - 1))) < 1e-9 else lo
    hi = float(grid[round(hi * (timesteps - 1))]) if abs(hi * (timesteps - 1) - round(hi * (timesteps - 1))) < 1e-9 else hi
    got = vm.guidance_interval_weights(timesteps, lo, hi)
    assert got == [float(v) for v in want] and len(got) == len(vm.euler_tables(timesteps)[0])


def test_interval_weights_on_the_50_step_table():
    w = vm.guidance_interval_weights(51, 0.25, 0.75)
    grid = torch.linspace(0, 1, 51)
    assert len(w) == 50 and set(w) <= {0.0, 1.0}
    assert w == [1.0 if np.float32(0.25) <= np.float32(t) <= np.float32(0.75) else 0.0 for t in grid[:-1].tolist()]
    assert w[:13] == [0.0] * 13 and w[13] == 1.0 and w[37] == 1.0 and w[38:] == [0.0] * 12 and sum(w) == 25
    # ends that are grid points: included on both sides
    assert vm.guidance_interval_weights(51, float(grid[10]), float(grid[20])) == [0.0] * 10 + [1.0] * 11 + [0.0] * 29
    # t_start cuts the grid like euler_tables does
    assert vm.guidance_interval_weights(51, 0.25, 0.75, t_start=20) == w[20:]
    for bad in ((0.6, 0.4), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            vm.guidance_interval_weights(51, *bad)


def test_engine_validates_and_lays_out_the_schedule():
    from versband_amd.engine import DiTEngine
    gs, held = DiTEngine._guidance_struct([0.0, 1.0, 0.5, 16.0], 4)
    assert [gs.weight[k] for k in range(4)] == [0.0, 1.0, 0.5, 16.0] and held is not None
    gs, _ = DiTEngine._guidance_struct(torch.tensor([0.25, 1.0]), 2)
    assert [gs.weight[k] for k in range(2)] == [0.25, 1.0]
    assert DiTEngine._guidance_struct([1.0, 1, np.float32(1)], 3) == (None, None), "all ones is the plain call"
    for bad, exc, pat in (([1.0, 0.0], ValueError, "2 entries for 3 steps"), ([1.0, float("nan"), 0.0], ValueError, r"guidance\[1\]"),
                          ([1.0, 0.0, -0.5], ValueError, r"guidance\[2\]"), ([16.5, 0.0, 1.0], ValueError, r"guidance\[0\]"),
                          ([1.0, float("inf"), 1.0], ValueError, r"guidance\[1\]"), ([1.0, "a", 1.0], TypeError, "numbers"),
                          ([True, 1.0, 1.0], TypeError, "numbers"), (0.5, TypeError, "sequence")):
        with pytest.raises(exc, match=pat):
            DiTEngine._guidance_struct(bad, 3)


class _StubEngine:
    def __init__(self):
        self.calls = []

    def sample_cfg(self, x0, pc, idx, dts, scale, **kw):
        self.calls.append(kw)
        return x0, torch.stack([x0] * (len(idx) + 1))


def _sampler():
    eng = _StubEngine()
    model = SimpleNamespace(num_timesteps=1000, device=torch.device("cpu"), sigma_min=1e-4, channels=0, _precompute=lambda conds, T: {"n": len(conds)},
                            dit_engine=lambda: eng)
    return vm.CFMSampler(model, 1000), eng


def test_sampler_hands_the_schedule_to_the_engine():
    s, eng = _sampler()
    x = torch.zeros(2, 20, 16)
    common = dict(cond={}, unconditional_guidance_scale=3.0, unconditional_conditioning={}, batch_size=2, timesteps=5, shape=[20, 16], x_latent=x, seed=1)
    s.sample_cfg(**common)
    s.sample_cfg(**common, guidance_weights=[1.0] * 4)
    s.sample_cfg(**common, guidance_interval=(0.0, 1.0))
    assert all("guidance" not in kw for kw in eng.calls), "None, all ones and an interval over every step are the plain call"
    s.sample_cfg(**common, guidance_weights=[0.0, 1.0, 0.5, 2])
    s.sample_cfg(**common, guidance_interval=(0.25, 0.5))
    s.sample_cfg(**common, guidance_weights=torch.tensor([0.0, 0.0, 0.0, 0.0]))
    assert [kw.get("guidance") for kw in eng.calls[3:]] == [[0.0, 1.0, 0.5, 2.0], [0.0, 1.0, 1.0, 0.0], [0.0] * 4]
    n = len(eng.calls)
    for kw, exc, pat in ((dict(guidance_weights=[1.0] * 4, guidance_interval=(0.0, 1.0)), ValueError, "at most one"),
                         (dict(guidance_weights=[1.0, 0.0, 1.0]), ValueError, "3 entries for 4 steps"),
                         (dict(guidance_weights=[1.0, float("nan"), 1.0, 1.0]), ValueError, r"guidance_weights\[1\]"),
                         (dict(guidance_weights=[1.0, 1.0, -1.0, 1.0]), ValueError, r"guidance_weights\[2\]"),
                         (dict(guidance_weights=[1.0, 1.0, 1.0, 17.0]), ValueError, r"guidance_weights\[3\]"),
                         (dict(guidance_interval=(0.7, 0.2)), ValueError, "lo <= hi"), (dict(guidance_interval=0.5), ValueError, r"\(lo, hi\)")):
        with pytest.raises(exc, match=pat):
            s.sample_cfg(**common, **kw)
    assert len(eng.calls) == n, "a refused schedule reaches no engine"
    with pytest.raises(TypeError):
        s.sample_cfg({}, 3.0, {}, 2, 5, [20, 16], x, None, None, 1, 0, None, None, None, None, [1.0] * 4)     # keyword-only


def test_long_form_passes_the_schedule_through():
    import inspect
    from versband_amd import longform
    assert inspect.signature(longform.sample_long).parameters["guidance"].default is None
    src = inspect.getsource(longform)
    assert src.count("**gk)") == 4, "crossfade, joint (two calls) and continue all hand the schedule on"


def test_cli_parses_the_interval_and_hands_it_to_guided_calls(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import infer_batched as ib
    assert ib.parse_interval("0.25-0.75") == (0.25, 0.75) and ib.parse_interval("0-1") == (0.0, 1.0)
    import argparse
    for bad in ("0.5", "a-b", "0.6-0.4", "-0.1-0.5", "0-1.5"):
        with pytest.raises(argparse.ArgumentTypeError):
            ib.parse_interval(bad)
    args = ib.parse_args(["--synthetic", "2", "--scales", "1-3", "--guidance_interval", "0.25-0.75"])
    assert args.guidance_interval == (0.25, 0.75)
    assert ib.parse_args(["--synthetic", "2"]).guidance_interval is None
    # the calls of one group: the guided call carries the interval, the scale-1.0 call stays the one-branch call it is
    seen = []

    class Sampler:
        model = SimpleNamespace(first_stage_model=SimpleNamespace(embed_dim=20), get_learned_conditioning=lambda c: c,
                                decode_first_stage=lambda z: torch.zeros(z.shape[0], 80, 2 * z.shape[-1]))

        def sample_cfg(self, **kw):
            seen.append(kw)
            return kw["x_latent"], None

    vocoder = SimpleNamespace(spec2wav_batch=lambda mel: torch.zeros(mel.shape[0], 8))
    item = {"midi": torch.zeros(1, 32), "beats": torch.zeros(1, 32), "acoustic": torch.zeros(80, 32), "caption": torch.zeros(4), "uncond_caption": torch.zeros(4),
            "name": "a"}
    args = SimpleNamespace(n_samples=1, seed=0, items_per_batch=1, ddim_steps=4, guidance_interval=(0.25, 0.75))
    ib.sample_group(args, Sampler(), vocoder, [(0, item)], [1.0, 3.0], torch.device("cpu"))
    assert len(seen) == 2
    for kw in seen:
        if kw["unconditional_conditioning"] is None:
            assert "guidance_interval" not in kw
        else:
            assert kw["guidance_interval"] == (0.25, 0.75)
    seen.clear()
    args.guidance_interval = None
    ib.sample_group(args, Sampler(), vocoder, [(0, item)], [1.0, 3.0], torch.device("cpu"))
    assert len(seen) == 2 and all("guidance_interval" not in kw for kw in seen)
