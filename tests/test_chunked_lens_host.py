"""The chunked vocoder with row lengths, host side (no GPU): the library's plan (vb_hifigan_chunked_lens_plan - the function the entry
point runs) against its Python mirror (harness.plan_chunk_calls), the properties of the plan, the refusals and the declarations.  The GPU
half is tests/test_gpu_chunked_lens.py."""
import ctypes as C
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

from versband_amd import _lib as L
from versband_amd import harness, longform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHUNKS = 256
# (T, chunk, halo, lengths): the cases of the GPU tests, rows that end inside a chunk / inside a trailing halo / before a chunk begins, a
# padded T longer than every row (a chunk without active rows), the one-step rule on both sides of T = chunk + 2 halo, halo 0, chunk 1
GRID = [
    (56, 16, 16, [56, 52, 40, 36, 20, 12, 4]),
    (54, 16, 16, [54, 47, 33, 21, 9]),
    (120, 40, 32, [120, 96, 44]),
    (24, 8, 4, [24] + [1 + (7 * b) % 24 for b in range(63)]),
    (24, 8, 4, [5]),
    (64, 16, 4, [30, 17, 16, 1]),
    (48, 16, 16, [48, 20, 3]),
    (49, 16, 16, [49, 20, 3]),
    (40, 10, 0, [40, 31, 30, 29, 10, 9]),
    (9, 1, 2, [9, 5, 1]),
    (6000, 3000, 32, [3600, 4400, 5200, 6000]),
]


def _random_cases(n=200, seed=20240607):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        B, T = rng.randint(1, 8), rng.randint(1, 200)
        chunk, halo = rng.randint(1, 80), rng.randint(0, 40)
        lens = [rng.randint(1, T) for _ in range(B)]
        if rng.random() < 0.3:
            lens[rng.randrange(B)] = T
        out.append((T, chunk, halo, lens))
    return out


@pytest.fixture(scope="module")
def lib():
    return L.load()


def lib_plan(lib, T, chunk, halo, lens, max_chunks=MAX_CHUNKS):
    """(rc, message, steps in the form of harness.plan_chunk_calls) from the library"""
    B = len(lens)
    arr = (C.c_int32 * B)(*lens)
    s, lo, tc, na = ((C.c_int32 * max(1, max_chunks))() for _ in range(4))
    rows, n = ((C.c_int32 * (max(1, max_chunks) * 64))() for _ in range(2))
    nc = C.c_int(-1)
    rc = lib.vb_hifigan_chunked_lens_plan(B, T, chunk, halo, arr, max_chunks, s, lo, tc, na, rows, n, C.byref(nc))
    if rc != 0:
        return rc, lib.vb_last_error(), nc.value
    steps = []
    for k in range(nc.value):
        for j in range(64):
            assert (rows[k * 64 + j], n[k * 64 + j]) == (-1, 0) or j < na[k], "entries behind n_active are (-1, 0)"
        steps.append({"s": s[k], "e": s[k + 1] if k + 1 < nc.value else T, "lo": lo[k], "tc": tc[k],
                      "rows": [rows[k * 64 + j] for j in range(na[k])], "n": [n[k * 64 + j] for j in range(na[k])]})
    return rc, b"", steps


def check_properties(T, chunk, halo, lens, steps):
    covered = {b: [] for b in range(len(lens))}
    whole = T <= chunk + 2 * halo
    assert [c["s"] for c in steps] == ([0] if whole else list(range(0, T, chunk))), "the grid of the plain loop"
    for c in steps:
        s, e, lo = c["s"], c["e"], c["lo"]
        assert e == (T if whole else min(s + chunk, T)) and lo == (0 if whole else max(0, s - halo))
        assert c["rows"] == [b for b, v in enumerate(lens) if v > s], "active rows: exactly those with len > s, ascending"
        assert c["tc"] == max(c["n"], default=0) and lo + c["tc"] <= T
        for b, n in zip(c["rows"], c["n"]):
            assert n == (lens[b] if whole else min(lens[b], s + chunk + halo) - lo) and 1 <= n <= c["tc"]
            keep = (s, min(e, lens[b]))
            assert keep[0] < keep[1], "an active row keeps a non-empty range"
            assert keep[1] - lo <= n, "the kept frames lie inside the row's frames of the chunk"
            covered[b].append(keep)
    for b, v in enumerate(lens):
        ranges = covered[b]
        assert ranges[0][0] == 0 and ranges[-1][1] == v, "the kept ranges of a row tile [0, len)"
        assert all(a[1] == nxt[0] for a, nxt in zip(ranges, ranges[1:])), "exactly once: each range starts where the last ended"


@pytest.mark.parametrize("case", GRID, ids=lambda c: f"T{c[0]}-c{c[1]}-h{c[2]}-B{len(c[3])}")
def test_library_plan_equals_the_python_mirror_on_the_grid(lib, case):
    T, chunk, halo, lens = case
    rc, msg, steps = lib_plan(lib, T, chunk, halo, lens)
    assert rc == 0, msg
    assert steps == harness.plan_chunk_calls(lens, T, chunk, halo)
    check_properties(T, chunk, halo, lens, steps)


def test_library_plan_equals_the_python_mirror_on_random_cases(lib):
    for T, chunk, halo, lens in _random_cases():
        rc, msg, steps = lib_plan(lib, T, chunk, halo, lens)
        assert rc == 0, (T, chunk, halo, lens, msg)
        assert steps == harness.plan_chunk_calls(lens, T, chunk, halo), (T, chunk, halo, lens)
        check_properties(T, chunk, halo, lens, steps)


def test_main_case_of_the_gpu_test_has_the_chunks_it_is_described_with():
    steps = harness.plan_chunk_calls([56, 52, 40, 36, 20, 12, 4], 56, 16, 16)
    assert [len(c["rows"]) for c in steps] == [7, 5, 4, 2]
    assert [(c["s"], c["lo"], c["tc"]) for c in steps] == [(0, 0, 32), (16, 0, 48), (32, 16, 40), (48, 32, 24)]
    assert steps[1]["n"] == [48, 48, 40, 36, 20] and steps[3]["n"] == [24, 20]
    assert all(n % 4 == c["tc"] % 4 for c in steps for n in c["n"]), "multiples of 4 throughout: every chunk is bit-exact"
    mixed = harness.plan_chunk_calls([54, 47, 33, 21, 9], 54, 16, 16)
    assert any(n % 4 != c["tc"] % 4 for c in mixed for n in c["n"])


def test_all_full_lengths_give_the_grid_of_the_plain_loop(lib):
    for T, chunk, halo in ((56, 16, 16), (100, 30, 7), (9000, 3000, 32), (48, 16, 16), (7, 1, 0)):
        rc, msg, steps = lib_plan(lib, T, chunk, halo, [T] * 3)
        assert rc == 0, msg
        plain, s = [], 0
        if T <= chunk + 2 * halo:
            plain.append((0, T, 0, T))
        else:
            while s < T:                   # (the loop of vb_hifigan_forward_chunked / longform.vocode_chunked)
                e = min(T, s + chunk)
                lo, hi = max(0, s - halo), min(T, e + halo)
                plain.append((s, e, lo, hi - lo))
                s = e
        assert [(c["s"], c["e"], c["lo"], c["tc"]) for c in steps] == plain
        assert all(c["rows"] == [0, 1, 2] and c["n"] == [c["tc"]] * 3 for c in steps)


def test_refusals_name_the_row_or_the_limit(lib):
    for lens, words in (([24, 0, 12], (b"row 1", b"length 0")), ([24, 12, 25], (b"row 2", b"length 25")), ([12] * 65, (b"65 rows", b"1..64"))):
        rc, msg, _ = lib_plan(lib, 24, 8, 4, lens)
        assert rc == -1 and all(w in msg for w in words), msg
    for chunk, halo in ((0, 4), (8, -1)):
        rc, msg, _ = lib_plan(lib, 24, chunk, halo, [24, 12])
        assert rc == -1 and f"chunk={chunk} halo={halo}".encode() in msg, msg
    rc, msg, count = lib_plan(lib, 24, 2, 1, [24, 12], max_chunks=3)
    assert rc == -1 and b"12 chunks" in msg and count == 12
    for lens, text in (([24, 0, 12], "row 1 has length 0"), ([24, 12, 25], "row 2 has length 25"), ([12] * 65, "65 rows")):
        with pytest.raises(ValueError, match=text):
            harness.plan_chunk_calls(lens, 24, 8, 4)
    with pytest.raises(ValueError, match="chunk = 0"):
        harness.plan_chunk_calls([24], 24, 0, 4)


# ---------------------------------------------------------------------------------------------------------------- Python layers
class _TorchNet:
    """a stand-in vocoder without run_chunked: a causal-free 'generator' whose sample depends on its frame and both neighbours, so a
    missing halo or a read behind a row's end shows; run(lengths=) follows ConvNet.run's contract (zero tails, padding not read)"""
    out_ch, out_tmul = 1, 2

    def run(self, mel, lengths=None):
        B, _, T = mel.shape
        x = mel.double().clone()
        if lengths is not None:
            for b, n in enumerate(lengths):
                x[b, :, n:] = 0.0
        m = torch.nn.functional.pad(x.sum(1, keepdim=True), (1, 1))
        y = (m[:, :, :-2] + 2 * m[:, :, 1:-1] - m[:, :, 2:]).repeat_interleave(2, dim=2)
        if lengths is not None:
            for b, n in enumerate(lengths):
                y[b, :, 2 * n:] = 0.0
        return y.float()


def test_torch_fallback_of_vocode_chunked_takes_lengths():
    net, T, lens = _TorchNet(), 56, [56, 52, 37, 20, 4]
    mel = torch.arange(len(lens) * 3 * T, dtype=torch.float32).reshape(len(lens), 3, T).sin()
    pad = mel.clone()
    for b, n in enumerate(lens):
        pad[b, :, n:] = float("nan")
    wav = longform.vocode_chunked(net, pad, chunk=16, halo=2, lengths=lens)
    assert wav.shape == (len(lens), 1, 2 * T) and torch.isfinite(wav).all()
    for b, n in enumerate(lens):
        alone = net.run(mel[b:b + 1, :, :n])
        assert torch.equal(wav[b:b + 1, :, :2 * n], alone) and int(torch.count_nonzero(wav[b, :, 2 * n:])) == 0
    full = longform.vocode_chunked(net, mel, chunk=16, halo=2, lengths=[T] * len(lens))
    assert torch.equal(full, longform.vocode_chunked(net, mel, chunk=16, halo=2))
    with pytest.raises(ValueError, match=r"lengths\[1\] = 57"):
        longform.vocode_chunked(net, mel, chunk=16, halo=2, lengths=[56, 57, 1, 1, 1])


def test_vocode_chunked_hands_lengths_to_run_chunked_and_spec2wav_batch_hands_chunk_on():
    from versband_amd.model import HifiGAN
    seen = []
    net = SimpleNamespace(out_ch=1, out_tmul=2, run=lambda mel, **kw: seen.append(("run", kw)) or torch.zeros(mel.shape[0], 1, 2 * mel.shape[2]),
                          run_chunked=lambda mel, chunk, halo, **kw: seen.append(("chunked", chunk, halo, kw)) or torch.zeros(mel.shape[0], 1, 2 * mel.shape[2]))
    voc = object.__new__(HifiGAN)
    voc.net = lambda: net
    mel = torch.zeros(2, 80, 40)
    assert voc.spec2wav_batch(mel).shape == (2, 80) and seen == [("run", {})]
    assert voc.spec2wav_batch(mel, lengths=[40, 20], chunk=8, halo=4).shape == (2, 80)
    assert seen[1] == ("chunked", 8, 4, {"lengths": [40, 20]})
    voc.spec2wav_batch(mel, chunk=8, halo=4)
    assert seen[2] == ("chunked", 8, 4, {})
    voc.spec2wav_batch(mel, lengths=[40, 40], chunk=8)                    # every row full: the call without lengths, halo 32 by default
    assert seen[3] == ("run", {})


def test_run_chunked_states_the_library_rules_first():
    from versband_amd.engine import ConvNet
    net = object.__new__(ConvNet)
    net.ctx = SimpleNamespace(device=torch.device("cpu"), lib=None, handle=None)
    net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul = L.NET_VOCODER, 80, 1, 320, 1
    mel = torch.zeros(3, 80, 24)
    for lens, text in (([24, 0, 12], r"lengths\[1\] = 0 is not in \[1, T = 24\]"), ([24, 12, 25], r"lengths\[2\] = 25 is not in \[1, T = 24\]")):
        with pytest.raises(ValueError, match=text):
            net.run_chunked(mel, 8, 4, lengths=lens)
    with pytest.raises(ValueError, match=r"65 rows \(at most 64\)"):
        net.run_chunked(torch.zeros(65, 80, 24), 8, 4, lengths=[12] * 65)
    with pytest.raises(ValueError, match="chunk = 0"):
        net.run_chunked(mel, 0, 4, lengths=[24, 12, 12])


# ---------------------------------------------------------------------------------------------------------------- header
def test_header_declares_the_entry_points_and_the_binding_knows_them():
    text = open(os.path.join(ROOT, "include", "versband_hip.h")).read()
    assert re.search(r"size_t\s+vb_hifigan_chunked_lens_workspace_bytes\(vb_ctx\*\s*\w*,\s*int B,\s*int T,\s*int chunk,\s*int halo\);", text)
    assert re.search(r"int\s+vb_hifigan_forward_chunked_lens\(vb_ctx\*\s*\w*,\s*const float\*\s*mel,\s*int B,\s*int T,\s*int chunk,\s*int halo,\s*"
                     r"const vb_lens\*\s*lens,\s*float\*\s*wav,\s*void\*\s*ws,\s*float\*\s*scratch_in,\s*float\*\s*scratch_out,\s*void\*\s*stream\);", text)
    assert re.search(r"int\s+vb_hifigan_chunked_lens_plan\(int B,\s*int T,\s*int chunk,\s*int halo,\s*const int32_t\*\s*len,\s*int max_chunks,", text)
    assert len(L.PROTOTYPES["vb_hifigan_forward_chunked_lens"][1]) == 12
    assert len(L.PROTOTYPES["vb_hifigan_chunked_lens_workspace_bytes"][1]) == 5
    assert len(L.PROTOTYPES["vb_hifigan_chunked_lens_plan"][1]) == 13
