"""The conv-net programs, bit for bit (CPU): every builder at every precision, and the builders' A/B switches, emit the op list, the
buffer table and the packed weights recorded in tests/golden/net_programs.json - so that a change to the host side of the conv nets
(versband_amd/engine.py: NetBuilder and the four build_*) which is meant to leave the programs alone is checked in seconds, without a
GPU.  The builders run as in tests/test_net_ops.py: device "cpu", ConvNet stubbed out, the synthetic default configurations.

The digest of one program is a sha256 over: which, in_ch, out_ch, out_tmul, in_tmul; the list nb.bufs; per op every field of L.NetOp in
_fields_ order - integers as they are, floats as their float32 bytes, a pointer as the sha256 (dtype, shape, contiguous bytes) of the
tensor in nb.keep that it points to, null as 0.  A pointer to no kept tensor fails: nothing would keep that memory alive.

    python tests/test_net_programs_host.py --write      regenerates the fixture (only where a change of the programs is intended)
"""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_net_ops as net_ops
from versband_amd import _lib as L
from versband_amd import engine

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_programs.json")
BUILDERS = ("vae_decoder", "vae_encoder", "hifigan", "bigvgan")
PRECISIONS = ("split", "fp32", "fp32mf", "bf16", "bf16xt")
SWITCHES = ("VB_MF_PAIRS_OFF", "VB_FP32_PAIRS", "VB_LRELU_IN_WINDOW", "VB_FP32_NO_PREPASS", "VB_XT_MIN_CO", "GN_PREPASS_MIN_CO")

# case name -> (builder, precision, environment, keyword arguments of the builder)
CASES = {f"{name}-{precision}": (name, precision, {}, {}) for name in BUILDERS for precision in PRECISIONS}
CASES.update({
    "hifigan-fp32-VB_FP32_PAIRS=": ("hifigan", "fp32", {"VB_FP32_PAIRS": ""}, {}),
    "hifigan-fp32mf-VB_FP32_PAIRS=": ("hifigan", "fp32mf", {"VB_FP32_PAIRS": ""}, {}),
    "hifigan-fp32-VB_FP32_PAIRS=32,64": ("hifigan", "fp32", {"VB_FP32_PAIRS": "32,64"}, {}),
    "hifigan-fp32mf-VB_FP32_PAIRS=32,64": ("hifigan", "fp32mf", {"VB_FP32_PAIRS": "32,64"}, {}),
    "hifigan-fp32mf-VB_MF_PAIRS_OFF=1": ("hifigan", "fp32mf", {"VB_MF_PAIRS_OFF": "1"}, {}),
    "hifigan-fp32-VB_LRELU_IN_WINDOW=1": ("hifigan", "fp32", {"VB_LRELU_IN_WINDOW": "1"}, {}),
    "hifigan-split-nofuse-VB_LRELU_IN_WINDOW=1": ("hifigan", "split", {"VB_LRELU_IN_WINDOW": "1"}, {"fuse_pairs": ()}),   # (unfused pairs exist)
    "vae_decoder-fp32-VB_FP32_NO_PREPASS=1": ("vae_decoder", "fp32", {"VB_FP32_NO_PREPASS": "1"}, {}),
    "vae_decoder-fp32mf-VB_FP32_NO_PREPASS=1": ("vae_decoder", "fp32mf", {"VB_FP32_NO_PREPASS": "1"}, {}),
})


class _Program:
    """stands in for ConvNet (and for test_net_ops._Captured): keeps every argument of the constructor"""

    def __init__(self, ctx, which, nb, in_ch, out_ch, out_tmul, in_tmul=1):
        self.which, self.nb, self.in_ch, self.out_ch, self.out_tmul, self.in_tmul = which, nb, in_ch, out_ch, out_tmul, in_tmul


def _tensor_digest(t: torch.Tensor) -> str:
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.detach().cpu().contiguous().flatten().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def program_digest(net) -> str:
    nb = net.nb
    digest_of = functools.lru_cache(maxsize=None)(lambda i: _tensor_digest(nb.keep[i]))
    kept = {}
    for i, t in enumerate(nb.keep):
        kept.setdefault(t.data_ptr(), i)
    h = hashlib.sha256()
    h.update(repr([int(v) for v in (net.which, net.in_ch, net.out_ch, net.out_tmul, net.in_tmul)]).encode())
    h.update(repr([tuple(int(v) for v in b) for b in nb.bufs]).encode())
    for n, op in enumerate(nb.ops):
        for field, ctype in L.NetOp._fields_:
            v = getattr(op, field)
            if ctype is C.c_void_p:
                assert v is None or v in kept, f"op {n}: {field} points to no tensor of nb.keep"
                h.update(b"0" if v is None else digest_of(kept[v]).encode())
            elif ctype is C.c_float:
                h.update(C.c_float(v))
            else:
                assert ctype is C.c_int, (field, ctype)
                h.update(repr(int(v)).encode())
            h.update(b";")
    return h.hexdigest()


def _record(case: str, monkeypatch) -> dict:
    name, precision, env, kwargs = CASES[case]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(net_ops, "_Captured", _Program)
    if kwargs:
        monkeypatch.setattr(engine, f"build_{name}", functools.partial(getattr(engine, f"build_{name}"), **kwargs))
    net = net_ops._build(name, precision, monkeypatch)
    return {"digest": program_digest(net), "ops": len(net.nb.ops)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_program_is_the_recorded_one(case, monkeypatch):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted(CASES)
    assert _record(case, monkeypatch) == want[case]


def test_xt_min_co_default():
    """VB_XT_MIN_CO is read when the module is imported: unset, wide layers start at 384 output channels"""
    assert engine.NetBuilder.XT_MIN_CO == int(os.environ.get("VB_XT_MIN_CO", 384))
    if "VB_XT_MIN_CO" not in os.environ:
        assert engine.NetBuilder.XT_MIN_CO == 384


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    got = {}
    for case_ in sorted(CASES):
        with pytest.MonkeyPatch.context() as mp:
            got[case_] = _record(case_, mp)
    with open(FIXTURE, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} programs -> {FIXTURE}")
