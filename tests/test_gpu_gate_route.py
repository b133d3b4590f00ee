"""The one-launch caption gate (gate_route.hip: scores, per-head softmax, value/gate contraction and routing of 64 tokens per workgroup,
lane-local in the MFMA's accumulator layout) against the two launches it replaces (grouped score GEMM + router_kernel): same MFMA k order,
same association order of every sum, the router's own phase B - so routes, gate weights, bucket tables and the DiT output must agree to
the bit.  VB_GATE_ROUTE=0 forces the two launches, =1 the one launch at every token count (the default picks by token count)."""
from __future__ import annotations

import pytest
import torch

from tests.helpers import SEED, clip_batch, describe, exp_noise, gumbel_arrays
from versband_amd import _lib as L
from versband_amd import model as vm
from versband_amd import synth

pytestmark = pytest.mark.gpu
LC, E = 80, 4
TWO, ONE = {"VB_GATE_ROUTE": "0"}, {"VB_GATE_ROUTE": "1"}


@pytest.fixture(scope="module")
def ctx():
    from versband_amd.engine import Context
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Context("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(synth.dit_shapes(synth.DiTConfig(num_experts=E)), SEED)


@pytest.fixture(scope="module")
def eng(ctx, sd):
    from versband_amd.engine import DiTEngine
    return DiTEngine(ctx, synth.DiTConfig(num_experts=E), sd, precision="bf16")


def under(monkeypatch, knobs, fn):
    """fn() with the knobs set; the environment and the library's copy of it are restored afterwards"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    L.load().vb_tune_reload()
    try:
        out = fn()
        torch.cuda.synchronize()
        return tuple(t.clone() for t in out) if isinstance(out, tuple) else out.clone()
    finally:
        for k in knobs:
            monkeypatch.delenv(k)
        L.load().vb_tune_reload()


def same(what, a, b):
    (v1, r1), (v2, r2) = a, b
    assert torch.isfinite(v1).all()
    assert torch.equal(r1, r2), f"{what}: routes differ at {(r1 != r2).sum().item()} of {r1.numel()} decisions"
    assert torch.equal(v1, v2), describe(what, v1, v2)


def inputs(eng, B, T, t=413):
    inp = clip_batch(B, T, LC)
    cond = eng.precompute_cond(torch.cat([inp["t5_cond"], inp["t5_uncond"]]), inp["midi"], inp["beats"], T)
    return inp, cond, torch.full((2 * B,), t, dtype=torch.int64)


@pytest.mark.parametrize("B,T", [(1, 64), (1, 65), (2, 100), (4, 752)])
def test_one_launch_matches_two_launches(eng, monkeypatch, B, T):
    """Exactly one tile; a one-token last tile; a ragged tile at every clip boundary (rows [B, 2B) are the second branch, another
    caption); the workload's length with several tiles per clip.  Routes of every block and the velocity, device-drawn and injected noise."""
    inp, cond, t_idx = inputs(eng, B, T)
    noise = gumbel_arrays([exp_noise(B, T, E, 0, 4), exp_noise(B, T, E, 1, 4)])
    for kw in (dict(seed=21, clip_base=3, nfe=2), dict(noise=noise)):
        fwd = lambda: eng.forward(inp["x_latent"], t_idx, cond, return_routes=True, **kw)
        same(f"one launch vs two, B={B} T={T} {sorted(kw)}", under(monkeypatch, ONE, fwd), under(monkeypatch, TWO, fwd))


def test_sampler_rows_with_their_own_clip_ids(eng, monkeypatch):
    """No C-ABI unit wrapper runs the router alone, so the per-row clip ids (non-consecutive, device-drawn noise keyed by them) are
    compared through the sampler: two guided Euler steps, graph replay included."""
    B, T = 3, 100
    inp, cond, _ = inputs(eng, B, T)
    idx, dts = vm.euler_tables(3)
    run = lambda: eng.sample_cfg(inp["x_latent"], cond, idx, dts, 3.0, seed=7, clip_ids=[11, 2, 40])
    z1, z2 = under(monkeypatch, ONE, run), under(monkeypatch, TWO, run)
    assert torch.isfinite(z1).all() and torch.equal(z1, z2), describe("sampler with clip ids, one launch vs two", z1, z2)


def test_near_ties_pick_the_same_first_maximum(ctx, sd, monkeypatch):
    """Experts 0 and 1 of the caption gate share their weights and bias in every block and two caption keys are the same row, so their
    logits are equal; the injected noise of expert 1 equals expert 0's on even tokens (an exact tie: the first maximum, never expert 1)
    and is one ulp above on odd tokens.  Both forms must decide alike."""
    from versband_amd.engine import DiTEngine
    sd2 = {k: v.clone() for k, v in sd.items()}
    tied = [k for k in sd2 if "caption_gating_network" in k]
    assert tied
    for k in tied:
        sd2[k][1] = sd2[k][0]
    eng2 = DiTEngine(ctx, synth.DiTConfig(num_experts=E), sd2, precision="bf16")
    B, T = 2, 100
    inp = clip_batch(B, T, LC)
    t5 = torch.cat([inp["t5_cond"], inp["t5_uncond"]]).clone()
    t5[:, 4] = t5[:, 3]
    cond = eng2.precompute_cond(t5, inp["midi"], inp["beats"], T)
    t_idx = torch.full((2 * B,), 413, dtype=torch.int64)
    g1, g2, g3 = gumbel_arrays([exp_noise(B, T, E, 0, 4), exp_noise(B, T, E, 1, 4)])
    g2 = g2.clone()
    g2[:, 0::2, 1] = g2[:, 0::2, 0]
    g2[:, 1::2, 1] = torch.nextafter(g2[:, 1::2, 0], torch.full_like(g2[:, 1::2, 0], float("inf")))
    fwd = lambda: eng2.forward(inp["x_latent"], t_idx, cond, return_routes=True, noise=(g1, g2, g3))
    one, two = under(monkeypatch, ONE, fwd), under(monkeypatch, TWO, fwd)
    same("near ties", one, two)
    ic = one[1][:, 0].cpu()
    assert not (ic[:, 0::2] == 1).any(), "an exact tie of experts 0 and 1 went to the second maximum"
    assert (ic[:, 1::2] == 1).any(), "one ulp above never won: the case does not exercise a near tie"


@pytest.mark.parametrize("B,T", [(4, 752), (3, 700), (2, 100)])
def test_count_table_matches_the_routers(eng, monkeypatch, B, T):
    """The bucket place kernel ranks from the per-256-token count table the router filled (N > 4096: 6016 and 4200 tokens, the second
    with ragged tiles and a partial last block; 400 tokens take the single-workgroup bucket kernel, no table).  A wrong table shows in
    perm / group_off / pair_off and so in the output: the one launch's table against router_kernel's and against bucket_count_kernel's."""
    inp, cond, t_idx = inputs(eng, B, T, t=250)
    fwd = lambda: eng.forward(inp["x_latent"], t_idx, cond, return_routes=True, seed=5)
    one = under(monkeypatch, ONE, fwd)
    same(f"counts, one launch vs router_kernel, B={B} T={T}", one, under(monkeypatch, TWO, fwd))
    same(f"counts, one launch vs count launch, B={B} T={T}", one, under(monkeypatch, {**ONE, "VB_BUCKET_COUNT_LAUNCH": "1"}, fwd))
    same(f"counts, second evaluation, B={B} T={T}", one, under(monkeypatch, ONE, fwd))
