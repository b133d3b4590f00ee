"""Host side of the per-row sampler call (vb_sample_cfg_rows): the binding of the new entry point, the validation of per-row scales and
clip ids in DiTEngine.sample_cfg, the planning of scripts/infer_batched.py --items_per_batch and its argument parsing.  No GPU."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from versband_amd import _lib as L
from versband_amd import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_entry_point_is_declared_bound_and_additive():
    """vb_sample_cfg_rows sits in the header and in PROTOTYPES, vb_rows matches its ctypes mirror field for field, the two older entry
    points keep their prototypes and the ABI version did not move"""
    src = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+vb_sample_cfg_rows\s*\(", code) and "vb_sample_cfg_rows" in L.PROTOTYPES
    blk = re.search(r"typedef struct \{([^}]*)\} vb_rows;", code).group(1)
    fields = re.findall(r"(const float\*|const int64_t\*)\s+([a-z0-9_]+)\s*;", blk)
    assert [n for _, n in fields] == [f[0] for f in L.Rows._fields_] == ["cfg_scale", "clip"]
    assert [f[1] for f in L.Rows._fields_] == [L.c_void_p, L.c_void_p]
    assert L.C.sizeof(L.Rows) == 2 * L.C.sizeof(L.c_void_p)
    keep, rows = L.PROTOTYPES["vb_sample_cfg_keep"][1], L.PROTOTYPES["vb_sample_cfg_rows"][1]
    assert len(rows) == len(keep) + 1 and rows[:11] == keep[:11] and rows[12:] == keep[11:]      # the rows block goes in before the keep block
    assert len(L.PROTOTYPES["vb_sample_cfg"][1]) == len(keep) - 1
    lib = L.load()
    assert hasattr(lib, "vb_sample_cfg_rows") and hasattr(lib, "vb_sample_cfg_keep") and lib.vb_abi_version() == 3
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct \{[^}]*\} vb_rows;", src, flags=re.S).group(1)
    for needle in ("fmaf(cfg_scale[b], v_c - v_u, v_u)", "v_u + cfg_scale[b] * (v_c - v_u)", "clip[b]", "POINTERS", "n_branch == 1", "noise->g1"):
        assert needle in doc, needle


def _stub(device="cpu"):
    """what DiTEngine._rows_struct needs of an engine: its device and the staging buffers (tests/test_keep_host.py's stubbing style)"""
    return SimpleNamespace(ctx=SimpleNamespace(device=torch.device(device)), cfg=SimpleNamespace(in_channels=20), _tables={}, _rowbuf={})


def test_engine_lays_out_the_row_block():
    from versband_amd.engine import DiTEngine
    eng = _stub()
    rs, scale, _ = DiTEngine._rows_struct(eng, 3.0, None, 3)
    assert rs is None and scale == 3.0, "a plain number is the scalar path"
    rs, scale, _ = DiTEngine._rows_struct(eng, np.float32(2.5), None, 3, clip_base=7)
    assert rs is None and scale == 2.5
    rs, scale, held = DiTEngine._rows_struct(eng, [1.5, 3, 4.5], (7, 2, 9), 3)
    assert scale == 0.0 and rs.cfg_scale == eng._rowbuf[(3, "scale")].data_ptr() and rs.clip == eng._rowbuf[(3, "clip")].data_ptr()
    assert eng._rowbuf[(3, "scale")].tolist() == [1.5, 3.0, 4.5] and eng._rowbuf[(3, "scale")].dtype == torch.float32
    assert eng._rowbuf[(3, "clip")].tolist() == [7, 2, 9] and eng._rowbuf[(3, "clip")].dtype == torch.int64
    before = (rs.cfg_scale, rs.clip)
    rs, _, _ = DiTEngine._rows_struct(eng, [2.0, 2.0, 2.0], [1, 2, 3], 3)
    assert (rs.cfg_scale, rs.clip) == before, "host values are staged into the same buffers: the graph key does not move"
    assert eng._rowbuf[(3, "clip")].tolist() == [1, 2, 3]
    # conforming tensors on the engine's device are passed as they are
    s, c = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([4, 5, 6])
    rs, scale, _ = DiTEngine._rows_struct(eng, s, c, 3)
    assert (rs.cfg_scale, rs.clip) == (s.data_ptr(), c.data_ptr()) and scale == 0.0
    rs, scale, _ = DiTEngine._rows_struct(eng, 3.0, c, 3)
    assert not rs.cfg_scale and rs.clip == c.data_ptr() and scale == 3.0
    rs, scale, _ = DiTEngine._rows_struct(eng, s, None, 3)
    assert rs.cfg_scale == s.data_ptr() and not rs.clip
    # ... and are not read (a read would be a device-to-host sync in front of every graph replay): their contents are the caller's contract
    inf = torch.tensor([1.0, float("inf"), 2.0])
    rs, _, _ = DiTEngine._rows_struct(eng, inf, None, 3)
    assert rs.cfg_scale == inf.data_ptr()


def test_engine_validates_rows_before_the_library_is_touched():
    """every refusal names its argument and comes from sample_cfg itself before anything is launched: the stand-in engine has no library,
    no workspace and no conditioning check to fall back on"""
    from versband_amd.engine import DiTEngine
    B = 3
    s, c = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([4, 5, 6])
    bad = [(dict(scale=[1.0, 2.0]), ValueError, r"scale has 2 entries for 3 rows"),
           (dict(scale=s[:2]), ValueError, r"scale has shape \(2,\)"),
           (dict(scale=s.reshape(3, 1)), ValueError, r"scale has shape"),
           (dict(scale=[1.0, float("nan"), 2.0]), ValueError, "scale must be finite"),
           (dict(scale=[1.0, float("inf"), 2.0]), ValueError, "scale must be finite"),
           (dict(scale=s.double()), TypeError, "scale must be float32"),
           (dict(scale=c), TypeError, "scale must be float32"),
           (dict(scale=["a", "b", "c"]), TypeError, "scale must hold numbers"),
           (dict(scale=None), TypeError, "scale must be a number, a sequence or a float32 tensor of 3 values"),
           (dict(scale=3.0, clip_ids=[1, 2]), ValueError, r"clip_ids has 2 entries for 3 rows"),
           (dict(scale=3.0, clip_ids=c[:2]), ValueError, r"clip_ids has shape \(2,\)"),
           (dict(scale=3.0, clip_ids=[1.0, 2.0, 3.0]), TypeError, "clip_ids must hold integers"),
           (dict(scale=3.0, clip_ids=[True, False, True]), TypeError, "clip_ids must hold integers"),
           (dict(scale=3.0, clip_ids=c.int()), TypeError, "clip_ids must be int64"),
           (dict(scale=3.0, clip_ids=s), TypeError, "clip_ids must be int64"),
           (dict(scale=3.0, clip_ids=7), TypeError, "clip_ids must be a sequence or an int64 tensor of 3 values"),
           (dict(scale=3.0, clip_ids=c, clip_base=4), ValueError, "clip_ids and a non-zero clip_base")]
    if not torch.cuda.is_available():
        bad += [(dict(scale=torch.empty(3, device="meta")), ValueError, "scale lives on"),
                (dict(scale=3.0, clip_ids=torch.empty(3, dtype=torch.int64, device="meta")), ValueError, "clip_ids lives on")]
    cond = {"B": B, "nb": 2, "T": 16, "L": 8}
    for kw, exc, pat in bad:
        eng = _stub()
        eng._rows_struct = lambda *a, **k: DiTEngine._rows_struct(eng, *a, **k)
        with pytest.raises(exc, match=pat):
            DiTEngine.sample_cfg(eng, torch.zeros(B, 20, 16), cond, [0, 500], [0.5, 0.5], **kw)


def test_sampler_forwards_scales_and_clip_ids():
    """CFMSampler.sample_cfg / sample hand a per-row scale and clip_ids to the engine unchanged, a plain number as a float"""
    from versband_amd import model as vm
    seen = []

    class Eng:
        def sample_cfg(self, x0, pc, idx, dts, scale, noise=None, seed=0, clip_base=0, return_traj=False, keep=None, clip_ids=None):
            seen.append((scale, clip_ids, clip_base))
            return x0, torch.stack([x0, x0])

    m = SimpleNamespace(num_timesteps=1000, sigma_min=1e-4, device=torch.device("cpu"), channels=0, mel_dim=20, mel_length=16,
                        _precompute=lambda conds, T: {"n": len(conds)}, dit_engine=lambda: Eng())
    s = vm.CFMSampler(m, 1000)
    x = torch.zeros(2, 20, 16)
    scales = torch.tensor([1.5, 3.0])
    s.sample_cfg({}, scales, {}, batch_size=2, timesteps=4, shape=(20, 16), x_latent=x, seed=1, clip_ids=[5, 9])
    s.sample_cfg({}, [1.5, 3.0], {}, batch_size=2, timesteps=4, shape=(20, 16), x_latent=x, seed=1)
    s.sample_cfg({}, 3, {}, batch_size=2, timesteps=4, shape=(20, 16), x_latent=x, seed=1, clip_base=4)
    s.sample({}, batch_size=2, timesteps=4, shape=(20, 16), x_latent=x, seed=1, clip_ids=[5, 9])
    assert seen[0][0] is scales and seen[0][1] == [5, 9]
    assert seen[1] == ([1.5, 3.0], None, 0)
    assert seen[2] == (3.0, None, 4) and isinstance(seen[2][0], float)
    assert seen[3] == (1.0, [5, 9], 0)


# ---------------------------------------------------------------------------------------------------------------- planning
CASES = [([75, 75, 115, 75], [1.0, 3.0, 4.5], 2, 4),
         ([75] * 9, [3.0], 1, 4),
         ([75, 75, 75, 100, 100, 75], [1.0], 3, 2),
         ([60, 61, 62], [1.0, 2.0], 1, 8),
         ([75] * 5, [1.0, 3.0], 2, 1),
         ([], [3.0], 1, 4)]


@pytest.mark.parametrize("lengths,scales,n,ipb", CASES)
def test_plan_row_batches_covers_every_row_once_in_order(lengths, scales, n, ipb):
    indices = [3 + 2 * p for p in range(len(lengths))]                 # a rank's shard: global indices rank::world
    calls = harness.plan_row_batches(lengths, scales, n, ipb, indices)
    rows = [r for c in calls for r in c["rows"]]
    assert sorted(rows) == sorted((p, s, k) for p in range(len(lengths)) for s in scales for k in range(n)), "every (item, scale, sample) exactly once"
    last_item = -1
    for c in calls:
        assert c["items"] == sorted(c["items"]) and c["items"] == list(range(c["items"][0], c["items"][-1] + 1)), "consecutive items in shard order"
        assert {lengths[p] for p in c["items"]} == {c["length"]}, "a call never mixes lengths"
        assert len(c["items"]) <= ipb and len(c["rows"]) <= harness.MAX_ROWS_PER_CALL
        assert c["n_branch"] == (1 if all(s == 1.0 for _, s, _ in c["rows"]) else 2)
        assert all((s == 1.0) == (c["n_branch"] == 1) for _, s, _ in c["rows"]), "guided and unguided rows never share a call"
        assert c["clip_ids"] == [indices[p] * n + k for p, _, k in c["rows"]]
        assert [p for p, _, _ in c["rows"]] == sorted(p for p, _, _ in c["rows"]), "rows are item-major"
        for p in c["items"]:                                            # the samples of one (item, scale) are a run, scales in the order given
            mine = [(s, k) for q, s, k in c["rows"] if q == p]
            assert mine == [(s, k) for s in scales if (s == 1.0) == (c["n_branch"] == 1) for k in range(n)]
        assert c["items"][0] >= last_item, "groups come in shard order"
        last_item = c["items"][0]
    if ipb > 1:
        for a, b in zip(calls, calls[1:]):                              # a group is as large as the cap and the lengths allow
            if a["n_branch"] == b["n_branch"] and a["length"] == b["length"] and b["items"][0] == a["items"][-1] + 1:
                assert len(a["items"]) == ipb
        per_group = {}
        for c in calls:
            per_group.setdefault(tuple(c["items"]), []).append(c["n_branch"])
        want = ([2] if any(s != 1.0 for s in scales) else []) + ([1] if 1.0 in scales else [])
        assert all(v == want for v in per_group.values()), "ONE guided and one unguided call per group"


@pytest.mark.parametrize("lengths,scales,n,ipb", CASES)
def test_planning_group_by_group_is_the_whole_plan(lengths, scales, n, ipb):
    """the CLI forms one group at a time from a lazy stream of items (stream_groups) and plans that group alone: the calls are those of
    the plan over the whole shard, and an item is not pulled from the stream before the previous group is complete"""
    indices = [3 + 2 * p for p in range(len(lengths))]
    pulled = []

    def stream():
        for p in range(len(lengths)):
            pulled.append(p)
            yield p

    calls, start = [], 0
    for group in harness.stream_groups(stream(), lengths.__getitem__, ipb):
        assert group == list(range(start, start + len(group))) and max(pulled) <= group[-1] + 1, "at most one item of the next group is read"
        part = harness.plan_row_batches([lengths[p] for p in group], scales, n, ipb, [indices[p] for p in group])
        for c in part:
            calls.append(dict(c, items=[start + q for q in c["items"]], rows=[(start + q, s, k) for q, s, k in c["rows"]]))
        start += len(group)
    assert start == len(lengths) and calls == harness.plan_row_batches(lengths, scales, n, ipb, indices)


def test_items_per_batch_one_is_the_per_item_loop():
    """one call per (item, scale) in the loop's order, rows = the item's samples, keyed clip_base = gi * n_samples"""
    lengths, scales, n = [75, 100, 75], [1.0, 3.0, 4.5], 2
    calls = harness.plan_row_batches(lengths, scales, n, 1, [4, 5, 6])
    assert [(c["items"], c["rows"][0][1], c["n_branch"]) for c in calls] == [([p], s, 1 if s == 1.0 else 2) for p in range(3) for s in scales]
    for c in calls:
        gi = [4, 5, 6][c["items"][0]]
        assert c["clip_ids"] == [gi * n + k for k in range(n)] and len(c["rows"]) == n and c["length"] == lengths[c["items"][0]]


def test_items_per_batch_is_checked_against_the_row_cap():
    harness.check_items_per_batch(4, [1.0, 3.0, 4.5], 2)               # 4 x 2 x 2 = 16 rows
    harness.check_items_per_batch(32, [3.0], 1)
    harness.check_items_per_batch(1, [1.0, 2.0, 3.0, 4.0, 5.0], 16)    # the loop itself is never refused
    with pytest.raises(ValueError, match=r"--items_per_batch 8 x 2 guided scales x 3 samples = 48 rows.*at most 32"):
        harness.check_items_per_batch(8, [1.0, 3.0, 4.5], 3)
    with pytest.raises(ValueError, match="33 rows"):
        harness.plan_row_batches([75] * 40, [3.0], 1, 33)
    with pytest.raises(ValueError, match="at least 1"):
        harness.check_items_per_batch(0, [3.0], 1)


def test_synthetic_frames_parses_one_length_or_a_cycle(monkeypatch):
    assert harness.parse_frames("150") == [150] and harness.parse_frames(150) == [150]
    assert harness.parse_frames("150,150,230,150") == [150, 150, 230, 150]
    for bad in ("", "150,", "a", "150,-3", "0"):
        with pytest.raises(ValueError, match="synthetic_frames"):
            harness.parse_frames(bad)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import infer_batched as cli
    finally:
        sys.path.pop(0)
    args = cli.parse_args(["--synthetic", "2", "--synthetic_frames", "150", "--scales", "1-3"])
    assert args.items_per_batch == 1 and args.synthetic_frames == [150] and args.synthetic == 2 and args.scales == "1-3"
    ds = cli.SyntheticDataset(3, args.synthetic_frames, 1234)
    assert [ds[i]["acoustic"].shape[1] for i in range(3)] == [152, 152, 152]
    ds = cli.SyntheticDataset(4, [150, 230], 1234)
    assert [ds[i]["acoustic"].shape[1] for i in range(4)] == [152, 232, 152, 232]
    one = cli.loop.SyntheticDataset(1, 150, 1234)[0]            # the loop's own dataset gives the same item for the same length
    assert all(torch.equal(ds[0][k], one[k]) for k in ("caption", "midi", "beats", "acoustic"))
    monkeypatch.setattr(sys, "argv", ["infer_batched.py"])
    args = cli.parse_args()
    assert args.synthetic_frames == [1500] and args.items_per_batch == 1 and args.ddim_steps == 24
    args = cli.parse_args(["--synthetic", "4", "--synthetic_frames", "150,150,230,150", "--items_per_batch", "4", "--n_samples", "2", "--scales", "1-3-4.5"])
    assert args.synthetic_frames == [150, 150, 230, 150] and args.items_per_batch == 4
    with pytest.raises(ValueError, match="rows per sampler call"):
        cli.parse_args(["--synthetic", "4", "--items_per_batch", "9", "--n_samples", "4"])
