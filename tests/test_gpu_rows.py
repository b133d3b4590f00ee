"""Per-row guidance scale and noise key on the GPU (vb_sample_cfg_rows, through the C ABI): rows that differ in guidance scale or whose
global clip indices are not contiguous share one sampler call, and each row is what its own call would have computed.

Every comparison here is bit for bit (torch.equal).  Every update form - scalar or per-row scale, fused into FinalLayer or a launch of
its own, with or without a known region - is the same two fused multiply-adds (fmaf(s, v_c - v_u, v_u), then fmaf(dt, e, x): one device
function, common.h:euler_cfg_update), a clip's network evaluation
does not depend on its batch slot (tests/test_gpu_keep.py), and the router noise is a counter-based function of (seed, global clip, ...):
nothing is left that could round differently."""
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import SEED, clip_batch, describe
from versband_amd import _lib as L
from versband_amd import model as vm
from versband_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 1e-4
SCALES, CLIPS = [1.5, 3.0, 4.5], [7, 2, 9]


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


def _known(shape, tag=0):
    g = torch.Generator().manual_seed(4321 + tag)
    return torch.randn(shape, generator=g)


def _cond(eng, inp, T, nb, sel=slice(None)):
    t5 = torch.cat([inp["t5_cond"][sel], inp["t5_uncond"][sel]]) if nb == 2 else inp["t5_cond"][sel]
    return eng.precompute_cond(t5, inp["midi"][sel], inp["beats"][sel], T)


def _keep_masks(B, T):
    """the masks of tests/test_gpu_keep.py::test_a_clip_does_not_depend_on_its_batch_slot"""
    mask = torch.zeros(B, T)
    mask[0, :10] = 1.0
    mask[1, 30:] = 1.0
    mask[2, 5:25] = 1.0
    mask[2, 25:28] = torch.tensor([0.75, 0.5, 0.25])
    return mask


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
@pytest.mark.parametrize("prec", ["bf16", "split"])
@pytest.mark.parametrize("form", ["plain", "keep", "one_branch"])
def test_rows_equal_their_solo_calls(engines, prec, form):
    """row b of a call with scales [1.5, 3, 4.5] and clip ids [7, 2, 9] equals the B = 1 call with the scalar scale s_b, clip_base = clip_b
    and that row's conditioning - plain, with a known region, and with one branch (ids only: there is nothing to guide)"""
    eng = engines[prec]
    B, T, Lc = 3, 40, 8
    inp = clip_batch(B, T, Lc)
    idx, dts = vm.euler_tables(4)
    times = vm.euler_times(4)
    nb = 1 if form == "one_branch" else 2
    x0, ref, mask = inp["x_latent"], _known(inp["x_latent"].shape), _keep_masks(B, T)
    keep = (ref, x0, mask, times, SIGMA) if form == "keep" else None
    scale = 1.0 if nb == 1 else SCALES
    rows = eng.sample_cfg(x0, _cond(eng, inp, T, nb), idx, dts, scale, seed=5, clip_ids=CLIPS, keep=keep)
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all()
    for b in range(B):
        sel = slice(b, b + 1)
        k1 = (ref[sel].contiguous(), x0[sel].contiguous(), mask[sel].contiguous(), times, SIGMA) if keep else None
        solo = eng.sample_cfg(x0[sel], _cond(eng, inp, T, nb, sel), idx, dts, 1.0 if nb == 1 else SCALES[b], seed=5, clip_base=CLIPS[b], keep=k1)
        torch.cuda.synchronize()
        assert torch.equal(rows[sel], solo), describe(f"{form} {prec}: row {b} vs its solo call", rows[sel], solo)
    # the ids and the scales are honoured at all: the contiguous / uniform call is another result
    other = eng.sample_cfg(x0, _cond(eng, inp, T, nb), idx, dts, 1.0 if nb == 1 else 3.0, seed=5, clip_base=7, keep=keep)
    torch.cuda.synchronize()
    assert not torch.equal(rows[1], other[1]), "row 1 is clip 2 here and clip 8 there"
    if nb == 1:
        assert torch.equal(rows[0], other[0]) and torch.equal(rows[2], other[2]), "rows 0 and 2 are clips 7 and 9 in both calls"
    else:
        assert not torch.equal(rows[0], other[0]) and not torch.equal(rows[2], other[2]), "rows 0 and 2 are guided by 1.5 and 4.5, not 3"


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("launch", ["fused", "VB_EULER_LAUNCH"])
@pytest.mark.parametrize("with_keep", [False, True])
def test_uniform_rows_equal_the_scalar_call(engines, knobs, launch, with_keep):
    """scales [3, 3, 3] with ids [5, 6, 7] are the scalar call with clip_base = 5: in the fused update and under VB_EULER_LAUNCH=1 (the
    separate launches, each per-row kernel against its scalar form), at every step of the trajectory"""
    eng = engines["bf16"]
    B, T, Lc = 3, 40, 8
    inp = clip_batch(B, T, Lc)
    idx, dts = vm.euler_tables(4)
    x0 = inp["x_latent"]
    keep = (_known(x0.shape), x0, _keep_masks(B, T), vm.euler_times(4), SIGMA) if with_keep else None
    if launch != "fused":
        knobs(**{launch: "1"})
    cond = _cond(eng, inp, T, 2)
    xs, ts = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=5, clip_base=5, return_traj=True, keep=keep)
    xr, tr = eng.sample_cfg(x0, cond, idx, dts, [3.0, 3.0, 3.0], seed=5, clip_ids=[5, 6, 7], return_traj=True, keep=keep)
    plain = eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=5, clip_base=5, keep=keep)
    rows = eng.sample_cfg(x0, cond, idx, dts, torch.full((3,), 3.0), seed=5, clip_ids=torch.tensor([5, 6, 7]), keep=keep)
    torch.cuda.synchronize()
    assert torch.isfinite(ts).all() and ts.shape == tr.shape == (4, B, 20, T)
    for k in range(4):
        assert torch.equal(ts[k], tr[k]), describe(f"{launch} keep={with_keep}: state {k}", tr[k], ts[k])
    assert torch.equal(xs, xr) and torch.equal(plain, rows) and torch.equal(plain, xs)
    knobs()
    if launch != "fused":       # ... and the separate launches give what the fused launch gives, per-row like scalar
        fused = eng.sample_cfg(x0, _cond(eng, inp, T, 2), idx, dts, [3.0, 3.0, 3.0], seed=5, clip_ids=[5, 6, 7], keep=keep)
        torch.cuda.synchronize()
        assert torch.equal(fused, rows), describe("per-row: fused vs separate launches", rows, fused)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("with_keep", [False, True])
def test_odd_length_takes_the_scale_of_each_token(engines, with_keep):
    """T = 37, B = 2: the fused launch's waves take two tokens, so one wave holds the last token of clip 0 and the first of clip 1 -
    a scale looked up per wave would guide one of them with the other's"""
    eng = engines["bf16"]
    B, T, Lc = 2, 37, 8
    inp = clip_batch(B, T, Lc)
    idx, dts = vm.euler_tables(4)
    x0 = inp["x_latent"]
    ref, mask = _known(x0.shape), _keep_masks(3, T)[1:].contiguous()
    keep = (ref, x0, mask, vm.euler_times(4), SIGMA) if with_keep else None
    scales, clips = [1.5, 4.5], [3, 11]
    rows = eng.sample_cfg(x0, _cond(eng, inp, T, 2), idx, dts, scales, seed=5, clip_ids=clips, keep=keep)
    torch.cuda.synchronize()
    for b in range(B):
        sel = slice(b, b + 1)
        k1 = (ref[sel].contiguous(), x0[sel].contiguous(), mask[sel].contiguous(), vm.euler_times(4), SIGMA) if keep else None
        solo = eng.sample_cfg(x0[sel], _cond(eng, inp, T, 2, sel), idx, dts, scales[b], seed=5, clip_base=clips[b], keep=k1)
        torch.cuda.synchronize()
        assert torch.equal(rows[sel], solo), describe(f"T = 37, row {b} vs its solo call", rows[sel], solo)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def router_case(engines):
    """the bf16 case of tests/test_gpu_path.py::test_router_forms_are_bit_identical (E = 4, B = 4, T = 752, 80 caption keys), sampled
    for three steps with non-contiguous clip ids under the default router form; computed once"""
    eng = engines["bf16"]
    B, T, Lc = 4, 752, 80
    inp = clip_batch(B, T, Lc)
    idx, dts = vm.euler_tables(4)
    args = dict(scale=[1.5, 3.0, 4.5, 2.0], clip_ids=[11, 3, 40, 4])
    base = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 2), idx, dts, args["scale"], seed=5, clip_ids=args["clip_ids"])
    torch.cuda.synchronize()
    return eng, inp, T, idx, dts, args, base.clone()


@pytest.mark.parametrize("knob", ["VB_ROUTER_TPW=1", "VB_ROUTER_TPW=4", "VB_ROUTER_GENERIC=1", "VB_SCORE_FUSED=1", "VB_MOE_UNFUSED=1", "VB_BAND_UNFUSED=1"])
def test_every_router_form_honours_the_clip_ids(router_case, knobs, knob):
    eng, inp, T, idx, dts, args, base = router_case
    name, _, val = knob.partition("=")
    knobs(**{name: val})
    got = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 2), idx, dts, args["scale"], seed=5, clip_ids=args["clip_ids"])
    torch.cuda.synchronize()
    assert torch.isfinite(base).all() and torch.equal(got, base), describe(f"per-row ids under {knob}", got, base)
    contiguous = eng.sample_cfg(inp["x_latent"], _cond(eng, inp, T, 2), idx, dts, args["scale"], seed=5, clip_base=11)
    torch.cuda.synchronize()
    assert torch.equal(contiguous[0], base[0]) and not torch.equal(contiguous[1:], base[1:]), "the ids were not read under this form"


# ---------------------------------------------------------------------------------------------------------------- 5
def test_graph_replays_with_rewritten_row_tensors(ctx, sd, engines, knobs):
    """the graph key holds the two POINTERS: rewriting the scale and id tensors in place and calling again replays one graph with the
    new values; a scalar call afterwards captures its own"""
    eng = _fresh(ctx, sd, engines)
    B, T, Lc = 3, 40, 8
    inp = clip_batch(B, T, Lc)
    idx, dts = vm.euler_tables(4)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).cuda()
    midi, beats, x0 = inp["midi"].cuda(), inp["beats"].cuda(), inp["x_latent"].cuda()
    values = [([1.5, 3.0, 4.5], [7, 2, 9]), ([2.0, 2.5, 1.25], [1, 30, 4]), ([4.0, 1.5, 3.0], [9, 9, 0])]
    scale_t, clip_t = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(stream):
        cond = eng.precompute_cond(t5, midi, beats, T, persistent=True)
        for s, c in values:
            scale_t.copy_(torch.tensor(s))
            clip_t.copy_(torch.tensor(c))
            out.append(eng.sample_cfg(x0, cond, idx, dts, scale_t, seed=5, clip_ids=clip_t))
        stream.synchronize()
        assert eng.graphs() == 1, "the repeated per-row call was not captured, or each call captured its own graph"
        plain = [eng.sample_cfg(x0, cond, idx, dts, 3.0, seed=5, clip_base=2) for _ in range(2)]
        stream.synchronize()
        assert eng.graphs() == 2, "a scalar call must capture its own graph, never replay the rows graph"
        # host values are staged into engine-owned buffers: they replay as well
        staged = [eng.sample_cfg(x0, cond, idx, dts, s, seed=5, clip_ids=c) for s, c in values]
        stream.synchronize()
        assert eng.graphs() == 3
    knobs(VB_NO_GRAPH="1")
    eager = _fresh(ctx, sd, engines)
    with torch.cuda.stream(stream):
        cond = eager.precompute_cond(t5, midi, beats, T, persistent=True)
        for i, (s, c) in enumerate(values):
            want = eager.sample_cfg(x0, cond, idx, dts, s, seed=5, clip_ids=c)
            stream.synchronize()
            assert torch.equal(out[i], want), describe(f"call {i} (graph) vs eager", out[i], want)
            assert torch.equal(staged[i], want), describe(f"staged call {i} vs eager", staged[i], want)
        want = eager.sample_cfg(x0, cond, idx, dts, 3.0, seed=5, clip_base=2)
        stream.synchronize()
    assert eager.graphs() == 0
    assert torch.equal(plain[0], want) and torch.equal(plain[1], want)
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_cli_batched_files_are_byte_identical(tmp_path):
    """scripts/infer_batched.py --items_per_batch 4 against 1 (the calls of the per-item loop, one per item and scale): same file lists, every .wav byte for byte, the same clap.csv (three scales incl. 1.0,
    two samples, items of two lengths: 150, 150, 230, 150 frames - the third item breaks the group)"""
    common = [sys.executable, os.path.join(ROOT, "scripts", "infer_batched.py"), "--synthetic", "4", "--synthetic_frames", "150,150,230,150",
              "--ddim_steps", "3", "--scales", "1-3-4.5", "--n_samples", "2"]
    listing = {}
    for ipb in ("4", "1"):
        out = tmp_path / "gen"                       # the same save_dir for both runs: clap.csv holds the paths
        r = subprocess.run(common + ["--items_per_batch", ipb, "--save_dir", str(out)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {}
        for d, _, names in os.walk(out):
            for nm in names:
                if nm.endswith(".wav") or nm == "clap.csv":
                    p = os.path.join(d, nm)
                    files[os.path.relpath(p, out)] = open(p, "rb").read()
                    os.remove(p)
        listing[ipb] = files
    a, b = listing["4"], listing["1"]
    assert sorted(a) == sorted(b) and len([f for f in a if f.endswith(".wav")]) == 4 * 3 * 2
    for name in sorted(a):
        assert a[name] == b[name], f"{name} differs between --items_per_batch 4 and 1"
    assert a["clap.csv"].count(b"\n") == 1 + 24


def test_cli_batched_files_are_those_of_the_entry_script(tmp_path):
    """scripts/infer_batched.py, batched and with --items_per_batch 1, against scripts/test_final.py itself on flags both accept: the
    per-item loop of the entry script is the yardstick, byte for byte"""
    common = ["--synthetic", "3", "--synthetic_frames", "150", "--ddim_steps", "3", "--scales", "1-3", "--n_samples", "2"]
    runs = {"loop": ["test_final.py"], "batched": ["infer_batched.py", "--items_per_batch", "3"], "one": ["infer_batched.py", "--items_per_batch", "1"]}
    listing = {}
    for name, (script, *extra) in runs.items():
        out = tmp_path / "gen"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + common + extra + ["--save_dir", str(out)],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        files = {}
        for d, _, names in os.walk(out):
            for nm in names:
                if nm.endswith(".wav") or nm == "clap.csv":
                    p = os.path.join(d, nm)
                    files[os.path.relpath(p, out)] = open(p, "rb").read()
                    os.remove(p)
        listing[name] = files
    want = listing["loop"]
    assert len([f for f in want if f.endswith(".wav")]) == 3 * 2 * 2
    for name in ("batched", "one"):
        assert sorted(listing[name]) == sorted(want)
        for f in sorted(want):
            assert listing[name][f] == want[f], f"{f}: {name} differs from scripts/test_final.py"
