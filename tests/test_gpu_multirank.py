"""BASELINE configs[3] (batch-shard over ranks) exercised on ONE GPU: `python bench.py --gpus 2` spawns its own two ranks
(VB_BENCH_ONE_DEVICE: both on cuda:0, gloo instead of RCCL for the weight broadcast), every rank generates its own clips,
and each clip must equal - bitwise - the clip a single process generates for the same global clip index: noise streams and
inputs are keyed by the global clip index, so the result is independent of world size (the reference shards the
same way with DistributedSampler, scripts/test_final.py:351-357,467-477)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra, timeout=900):
    env = dict(os.environ)
    env.update(env_extra)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    import tempfile
    detail = os.path.join(tempfile.mkdtemp(prefix="vb_bench_"), "bench_detail.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--detail", detail] + args, capture_output=True, text=True, timeout=timeout,
                       env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    # the driver's contract (round 5's 21 KB line came back `parsed: null`): the LAST stdout line is the one JSON object, <= 4 KB
    out_lines = r.stdout.strip().splitlines()
    lines = [ln for ln in out_lines if ln.startswith("{")]
    assert len(lines) == 1 and out_lines[-1] == lines[0], f"exactly one JSON line, last on stdout, expected; got {len(lines)}"
    assert len(lines[0]) <= 4096, len(lines[0])
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "config",
              "roofline", "detail"):
        assert k in line, k
    assert line["detail"] == detail
    full = json.load(open(detail))
    assert abs(full["value"] - line["value"]) <= 1e-5 * full["value"] and full["n_gpus"] == line["n_gpus"]
    assert line["config"]["workload"] == full["config"]["workload"]
    if full.get("parity_check") is not None:
        assert line["parity_check"]["ok"] == full["parity_check"]["ok"]
    return full


def test_two_ranks_one_command_match_single_process(tmp_path):
    common = ["--steps", "1", "--warmup", "1", "--flow-steps", "3", "--streams", "1", "--no-cpu-baseline", "--no-isolated"]
    d2, d1 = str(tmp_path / "w2"), str(tmp_path / "w1")
    out2 = _bench(["--gpus", "2", "--batch", "2", "--save-out", d2] + common, {"VB_BENCH_ONE_DEVICE": "1"})
    assert out2["n_gpus"] == 2 and out2["ranks"]["world"] == 2 and out2["ranks"]["weight_broadcast_bytes"] > 5e8
    assert out2["scaling"] == "weak" and out2["config"]["clips_per_gpu"] == 2
    out1 = _bench(["--gpus", "1", "--batch", "4", "--save-out", d1] + common, {})
    assert out1["n_gpus"] == 1
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) == [f"clip{i:04d}.npy" for i in range(4)]
    for n in names:
        a, b = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert a.shape == b.shape and np.isfinite(a).all()
        assert np.array_equal(a, b), f"{n}: rank-sharded output differs from the single-process output (max |d| = {np.abs(a - b).max():.3e})"


def test_c4_rank_shape_under_a_process_group():
    """configs[3]'s PER-RANK shape - 8 clips per rank as 2 concurrent sub-batches on 2 streams, the sampler loops replayed as
    hipGraphs - run by two ranks under a process group (one device, gloo): the JSON line must carry both ranks' timings, the
    broadcast rate, and the oracle verification of rank 0's clips."""
    out = _bench(["--gpus", "2", "--workload", "c2", "--batch", "8", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-isolated",
                  "--no-pmc"], {"VB_BENCH_ONE_DEVICE": "1"}, timeout=1500)
    assert out["n_gpus"] == 2 and out["config"]["clips_per_gpu"] == 8 and out["config"]["streams_per_gpu"] == 2
    assert len(out["ranks"]["per_rank_ms"]) == 2 and all(v > 0 for v in out["ranks"]["per_rank_ms"])
    assert out["ranks"]["weight_broadcast_gbps"] > 0 and out["ranks"]["collectives_in_timed_region"] == 0
    assert "hipGraph replay" in out["config"]["sampler_loop"]
    # rank 0 holds global clips 0..7: the fixture's clips 0, 4 (first clip of each sub-batch) and 7 (last row) x passes 0 and 1
    assert out["parity_check"]["ok"] is True and len(out["parity_check"]["verified"]["clips_x_passes"]) == 6
    # the default command times three VAE / vocoder arithmetics: `value` = fp32 with minimal filtering (configs[1]'s fp32 vocoder, round 6),
    # `fp32_direct` = the direct fp32 kernels (rounds 4-5's `value`), `split` = bf16x3 - each verified against the oracle
    assert out["config"]["vocoder_precision"] == "fp32mf"
    for key, prec in (("fp32_direct", "fp32"), ("split", "split")):
        assert out[key]["vocoder_precision"] == prec and out[key]["parity_check"]["ok"] is True and out[key]["value"] > 0
        assert len(out[key]["per_rank_ms"]) == 2


def test_cli_two_ranks_match_single_process(tmp_path):
    """The product entry point sharded over ranks (round 4: versband_amd/dist.py - rank::world item sharding, rank 0's checkpoints by one
    checked broadcast): `scripts/test_final.py --synthetic 4 --num_gpus 2` (both ranks on this one GPU, gloo) must write, for every item,
    the same PCM file a single process writes - noise, start latents and inputs are keyed by the global item index (the
    reference shards the same way, scripts/test_final.py:351-357,467-477)."""
    cli = os.path.join(ROOT, "scripts", "test_final.py")
    common = ["--synthetic", "4", "--synthetic_frames", "200", "--ddim_steps", "3", "--scales", "3", "--n_samples", "1"]

    def run(extra, env_extra):
        env = dict(os.environ)
        env.update(env_extra)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, cli] + common + extra, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        return r.stdout

    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    run(["--num_gpus", "1", "--save_dir", d1], {})
    out2 = run(["--num_gpus", "2", "--save_dir", d2, "--master_port", "54917"], {"VB_ONE_DEVICE": "1"})
    assert out2.count("model weights by broadcast") == 2 and "bitwise check passed" in out2

    def by_name(d, tags):
        m = {}
        for tag in tags:
            lines = open(os.path.join(d, f"clap{tag}.csv")).read().strip().splitlines()
            cols = lines[0].split("\t")
            for ln in lines[1:]:
                row = dict(zip(cols, ln.split("\t")))
                m[row["name"]] = row["audio_path"]
        return m
    one, two = by_name(d1, [""]), by_name(d2, [".0", ".1"])
    assert sorted(one) == sorted(two) == [f"synthetic{i:04d}" for i in range(4)]
    for name in one:
        a, b = open(one[name], "rb").read(), open(two[name], "rb").read()
        assert len(a) > 1000 and a == b, f"{name}: the rank-sharded run wrote a different waveform"


_RCCL_CHILD = r'''
import os, sys, json, torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from versband_amd import dist as vdist, synth
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[2]
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)        # "nccl" IS RCCL on ROCm
sd = synth.make_state_dict(synth.vae_decoder_shapes(synth.VAEConfig()), 7)
sd["an_int64"] = torch.arange(5)
sd["a_string"] = "kept"
out, info = vdist.broadcast_state(sd, src=0, device=dev, force=True)
ok = all(torch.equal(out[k].cpu(), v) for k, v in sd.items() if torch.is_tensor(v)) and out["a_string"] == "kept"
t = torch.ones(1 << 20, device=dev)
dist.all_reduce(t)
dist.barrier()
torch.cuda.synchronize()
print(json.dumps({"ok": bool(ok), "backend": dist.get_backend(), "info": {k: v for k, v in info.items()}, "allreduce": float(t[0]),
                  "on_device": all(v.is_cuda for v in out.values() if torch.is_tensor(v))}))
dist.destroy_process_group()
'''


def test_rccl_executes_the_weight_broadcast_in_a_one_rank_group():
    """Every N > 1 run so far was gloo on one device: RCCL itself had never executed.  Two ranks cannot share a GPU under
    RCCL, so this is the most a 1-GPU box can do: a process group of ONE rank on the nccl backend, versband_amd.dist.broadcast_state forced
    through its collectives (object broadcast of the layout, one flat device buffer per dtype through ncclBroadcast, all_gather of the
    checksums), an all_reduce and a barrier - the communicator is created on this GPU, the buffers are device memory, the state comes back
    bit for bit."""
    port = str(29500 + os.getpid() % 2000)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "VB_ONE_DEVICE", "VB_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD, ROOT, port], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    d = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert d["ok"] is True and d["backend"] == "nccl" and d["on_device"] is True and d["allreduce"] == 1.0
    assert d["info"]["backend"] == "nccl" and d["info"]["checked"] is True and d["info"]["buffers"] == 2 and d["info"]["bytes"] > 1e7
