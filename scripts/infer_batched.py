#!/usr/bin/env python3
"""AccompBand inference with batched sampler calls: the CLI of scripts/test_final.py plus `--items_per_batch N`.

scripts/test_final.py samples one item and one guidance scale per sampler call.  Here consecutive items of equal length, all their guided
scales and all their samples ride as rows of ONE call with a per-row guidance scale and noise key (vb_sample_cfg_rows, planned by
versband_amd.harness.plan_row_batches), and the batch is decoded and vocoded on the device.  The files - names, order, bytes, clap.csv - are
those of scripts/test_final.py.  The work goes group by group: a group's items are loaded, sampled, written and dropped before the next
group is formed, so memory does not grow with the manifest and a crash loses one group.  `--items_per_batch 1` (the default) makes the
calls of test_final.py's loop, one per (item, scale).  `--synthetic_frames` additionally accepts a comma list that cycles over the
synthetic items; every other flag is test_final.py's and is parsed by its parser.  `--length_slack N` lets consecutive items whose latent
lengths differ by at most N tokens share a call too: the group is padded to its longest member and sampled with per-row lengths
(vb_sample_cfg_lens - a row is the call on that clip alone), then the rows are decoded with per-row lengths (vb_vae_decode_lens) in one
call per residue of the latent length mod 4 and cut to their own lengths, and the decoded mels are vocoded with per-row lengths
(vb_hifigan_forward_lens) in one call per residue of the mel length mod 4 - two at most; in both a row again is the call on that clip alone.
`--eval_mel` scores a group's clips together: one MelNet call with row lengths (vb_melnet_forward_lens) over the written waveforms and one
masked distance reduction on the device (vb_mel_dist_lens); mel_l1.tsv keeps its columns and order, its values agree with the per-clip
path's to fp32 roundoff.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_final as loop  # noqa: E402
from versband_amd import dist as vdist  # noqa: E402
from versband_amd.harness import (MEL_DOWNSAMPLE, InferDataset, check_items_per_batch, parse_frames,  # noqa: E402
                                  plan_decode_calls, plan_row_batches, plan_vocoder_calls, save_rows_to_tsv, stream_length_groups, write_wav_pcm16)
from versband_amd.model import normalize_loudness  # noqa: E402


def parse_args(argv=None):
    """--items_per_batch, --synthetic_frames and --vocoder_precision are taken out of the command line here; every other flag goes through
    test_final.py's own parser (which reads sys.argv and is not ours to change: it sees the remaining arguments for the length of its call).
    --vocoder_precision is that parser's flag with two more choices, "bf16" and "bf16xt", the preview modes only this CLI offers."""
    from unittest import mock
    own = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    own.add_argument("--items_per_batch", type=int, default=1,
                     help="consecutive items of equal length that share ONE sampler call per group - all their guided scales and samples as "
                          "rows of one batch, decoded and vocoded on the device; the files are byte-identical to the per-item loop's "
                          "(default 1: that loop's calls).  items x guided scales x n_samples may not exceed 32 rows")
    own.add_argument("--length_slack", type=int, default=0,
                     help="latent tokens by which the items of one group may differ in length (default 0: equal lengths only, today's "
                          "grouping): consecutive items join a group while its longest member is at most this much longer than every "
                          "member; the group is sampled as one call padded to the longest, each row being the call on that clip alone")
    own.add_argument("--synthetic_frames", type=str, default="1500",
                     help="mel frames of a synthetic item: one integer, or a comma list that cycles over the items (150,150,230)")
    own.add_argument("--vocoder_precision", type=str, default="fp32mf", choices=["fp32mf", "fp32", "split", "bf16", "bf16xt"],
                     help="VAE + vocoder arithmetic: test_final.py's fp32mf (default) / fp32 / split, and bf16 = ONE bf16 pass per convolution (bf16 "
                          "operands, fp32 accumulation): preview quality, outside the 1e-3 parity bound; bf16xt = the same arithmetic with the wide "
                          "layers' inputs activated once into a bf16 plane and multiplied as DMA-fed GEMMs")
    own.add_argument("--guidance_interval", type=parse_interval, default=None, metavar="LO-HI",
                     help="guide only the steps that start at t in [LO, HI] (0-1 covers every step: today's files); the other steps of a "
                          "guided call evaluate the conditional branch alone.  The scale-1.0 rows stay the one-branch call they are")
    argv = list(sys.argv[1:] if argv is None else argv)
    if "-h" in argv or "--help" in argv:
        own.print_help()
        print("\n--eval_mel here scores a group's clips together: one MelNet call with row lengths over the written waveforms, one over the "
              "ground-truth accompaniments, and a device reduction (versband_amd.melnet.mel_distance) for the two mel_l1.tsv columns.  "
              "Its values agree with the per-clip torch reductions of scripts/test_final.py to 2 k 2^-24 (mean |d| + |offset|), "
              "k = ceil(80 * frames / 1024) + 10 - fp32 roundoff - not digit for digit; the .wav files and clap.csv are unchanged.")
        print("\nand every flag of scripts/test_final.py:\n")
    mine, rest = own.parse_known_args(argv)
    with mock.patch.object(sys, "argv", [sys.argv[0]] + rest):
        args = loop.parse_args()
    args.items_per_batch, args.synthetic_frames = mine.items_per_batch, parse_frames(mine.synthetic_frames)
    args.vocoder_precision = mine.vocoder_precision
    args.guidance_interval = mine.guidance_interval
    if mine.length_slack < 0:
        own.error(f"--length_slack must be at least 0, got {mine.length_slack}")
    args.length_slack = mine.length_slack
    check_items_per_batch(args.items_per_batch, list(dict.fromkeys(_scales(args))), args.n_samples)
    return args


def parse_interval(text):
    """"LO-HI" -> (lo, hi) with 0 <= lo <= hi <= 1"""
    try:
        lo, hi = (float(v) for v in text.split("-"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--guidance_interval {text!r}: expected LO-HI, two numbers in [0, 1]") from None
    if not 0.0 <= lo <= hi <= 1.0:
        raise argparse.ArgumentTypeError(f"--guidance_interval {text!r}: needs 0 <= LO <= HI <= 1")
    return lo, hi


def _scales(args):
    return [float(s) for s in args.scales.split("-")] if args.scales else [args.scale]


class SyntheticDataset:
    """test_final.py's synthetic items, item i with frames[i % len(frames)] mel frames"""

    def __init__(self, n, frames, seed):
        self.n, self.frames, self.seed = n, [int(f) for f in frames], seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return loop.SyntheticDataset(self.n, self.frames[i % len(self.frames)], self.seed)[i]


def _item_conditioning(sampler, item, n, device, guided):
    """the conditioning of one item's n samples as the per-item loop builds it: (cond, uncond or None)"""
    midi, beats, acoustic = item["midi"].to(device), item["beats"].to(device), item["acoustic"].to(device)
    cap = item["caption"]
    cond_in = {"caption": torch.stack([cap] * n) if torch.is_tensor(cap) else [cap] * n,
               "acoustic": {"acoustic": torch.stack([acoustic] * n), "midi": torch.stack([midi] * n).long(),
                            "beats": torch.stack([beats] * n).long()}, "name": [item["name"]] * n}
    c = sampler.model.get_learned_conditioning(cond_in)
    uc = None
    if guided:
        ucap = item.get("uncond_caption", "")
        uc_in = dict(cond_in)
        uc_in["caption"] = torch.stack([ucap] * n) if torch.is_tensor(ucap) else [ucap] * n
        uc = sampler.model.get_learned_conditioning(uc_in)
    return c, uc


def _cat_conditioning(parts, frames=None):
    """row-wise concatenation of learned conditionings (caption embeddings, index tracks, names); frames: the tracks of shorter items are
    zero-padded to that many mel frames first (a call with row lengths never reads the padding)"""
    def track(t):
        return t if frames is None or t.shape[-1] == frames else torch.nn.functional.pad(t, (0, frames - t.shape[-1]))
    return {"caption": torch.cat([c["caption"] for c in parts]),
            "acoustic": {k: torch.cat([track(c["acoustic"][k]) for c in parts]) for k in ("acoustic", "midi", "beats")},
            "name": [nm for c in parts for nm in c["name"]]}


def sample_group(args, sampler, vocoder, group, scales, device):
    """the sampler calls of harness.plan_row_batches for ONE group of items (of equal length, or within --length_slack of each other:
    the call then carries the row lengths, its rows are cut to them before decoding, and the vocoder call carries them again): group = [(global index, item)].  A row is what
    test_final.py computes for (item, scale, sample): the item's conditioning and start noise (the same for every scale of an item), its
    own guidance scale and its global clip index gi * n_samples + k as noise key - so the rows, and after the batched decode and vocoder
    the files, equal the loop's.  Returns {(position in the group, scale): [(mel [80,T], wav numpy)] per sample}."""
    n = args.n_samples
    embed_dim = sampler.model.first_stage_model.embed_dim
    indices, items = [gi for gi, _ in group], [it for _, it in group]
    lengths = [int(it["acoustic"].shape[1] / MEL_DOWNSAMPLE) for it in items]
    has_guided = any(s != 1.0 for s in scales)
    conds = [_item_conditioning(sampler, it, n, device, has_guided) for it in items]
    starts = [torch.randn(n, embed_dim, lengths[p], generator=torch.Generator().manual_seed(args.seed + gi)).to(device) for p, gi in enumerate(indices)]
    generated = {}
    for call in plan_row_batches(lengths, list(dict.fromkeys(scales)), n, args.items_per_batch, indices, getattr(args, "length_slack", 0)):
        rows = call["rows"]
        runs = [(p, s) for p, s, k in rows if k == 0]                          # rows come as runs of n samples of one (item, scale)
        row_lengths = call.get("row_lengths")                                  # None: one length, today's call
        frames = call["length"] * MEL_DOWNSAMPLE if row_lengths else None
        c = _cat_conditioning([conds[p][0] for p, _ in runs], frames)
        uc = _cat_conditioning([conds[p][1] for p, _ in runs], frames) if call["n_branch"] == 2 else None
        x = torch.cat([torch.nn.functional.pad(starts[p], (0, call["length"] - lengths[p])) if row_lengths else starts[p] for p, _ in runs])
        scale = [s for _, s, _ in rows] if call["n_branch"] == 2 else 1.0
        interval = getattr(args, "guidance_interval", None)
        gk = {"guidance_interval": interval} if interval is not None and call["n_branch"] == 2 else {}
        z, _ = sampler.sample_cfg(cond=c, unconditional_guidance_scale=scale, unconditional_conditioning=uc, batch_size=len(rows),
                                  shape=[embed_dim, call["length"]], x_latent=x, timesteps=args.ddim_steps + 1, seed=args.seed,
                                  clip_ids=call["clip_ids"], **gk, **({"lengths": row_lengths} if row_lengths else {}))
        done = {}
        if not row_lengths:
            mel = sampler.model.decode_first_stage(z)
            wav = vocoder.spec2wav_batch(mel).cpu().numpy()
            done.update({r: (mel[r], wav[r]) for r in range(len(rows))})
        else:
            # The VAE decoder and the vocoder take row lengths: the sampled latents are cut to the longest of their group
            # (harness.plan_decode_calls: lengths that agree mod 4, where a row equals the decode of that clip alone bit for bit), decoded
            # in one call and cut to their own lengths; the decoded mels are padded to the longest of their group
            # (harness.plan_vocoder_calls: mod 4), vocoded in one call and cut again
            mels = {}
            for dc in plan_decode_calls(row_lengths):
                zz = z[dc["rows"]][:, :, :dc["length"]].contiguous()
                mel = sampler.model.decode_first_stage(zz, **({"lengths": dc["lengths"]} if dc["lengths"] else {}))
                mels.update({r: mel[j, :, :row_lengths[r] * MEL_DOWNSAMPLE] for j, r in enumerate(dc["rows"])})
            for vc in plan_vocoder_calls([mels[r].shape[-1] for r in range(len(rows))]):
                batch = torch.stack([torch.nn.functional.pad(mels[r], (0, vc["length"] - mels[r].shape[-1])) for r in vc["rows"]])
                wav = vocoder.spec2wav_batch(batch, **({"lengths": vc["lengths"]} if vc["lengths"] else {})).cpu().numpy()
                hop = wav.shape[-1] // vc["length"]
                done.update({r: (mels[r], wav[j, :mels[r].shape[-1] * hop]) for j, r in enumerate(vc["rows"])})
        for r, (p, s, k) in enumerate(rows):
            generated.setdefault((p, s), []).append(done[r])
    return generated


def write_item(args, rank, item_idx, item, scales, generated, rows, pending, mel_net):
    """the files of one item in the per-item loop's order and under its names (test_final.py: gen_song, reference :424-457).  With
    --eval_mel every written clip is queued in `pending` - its mel_l1.tsv row without the values, the waveform as written, the decoded
    mel, the normalised ground-truth accompaniment or None - and the group is scored together by score_group."""
    cap = item["caption"]
    gt_vocal, gt_accomp = loop._load_ground_truth(item)
    for scale in scales:
        out_dir = os.path.join(args.save_dir, f"cond_gtcodec_accomp_scale_{scale}")
        for k, (spec, wav) in enumerate(generated[scale]):
            stem = os.path.join(out_dir, f"{rank}-{item_idx:04d}[{k}]")
            wav = normalize_loudness(wav, -23)
            if gt_vocal is not None:
                min_length = min(wav.shape[0], gt_vocal.shape[0])
                wav = wav[:min_length]
                gt_vocal = normalize_loudness(gt_vocal, -23)[:min_length]
                gt_accomp = normalize_loudness(gt_accomp, -23)
                write_wav_pcm16(stem + "[gt_vocal].wav", gt_vocal, args.sample_rate)
                write_wav_pcm16(stem + "[song].wav", wav[:min_length] + gt_vocal[:min_length], args.sample_rate)
                write_wav_pcm16(stem + "[gt_accomp].wav", gt_accomp, args.sample_rate)
            write_wav_pcm16(stem + "[accomp].wav", wav, args.sample_rate)
            rows.append({"audio_path": stem + "[accomp].wav", "caption": cap if isinstance(cap, str) else item["name"], "name": item["name"]})
            if mel_net is not None:
                pending.append(({"name": item["name"], "scale": scale, "sample": k}, np.asarray(wav, dtype=np.float32), spec,
                                None if gt_accomp is None else np.asarray(gt_accomp, dtype=np.float32)))


def _padded_rows(arrays, device):
    """1-D host arrays or [80, T] device mels of different lengths as the rows of one zero-padded device batch, and their lengths"""
    lens = [int(a.shape[-1]) for a in arrays]
    rows = [torch.nn.functional.pad(torch.as_tensor(a, dtype=torch.float32).to(device), (0, max(lens) - n)) for a, n in zip(arrays, lens)]
    return torch.stack(rows), lens


def score_group(pending, mel_net, mel_rows, device):
    """--eval_mel for the clips of one group (at most 64 per pass, the row limit of a call with lengths): the written waveforms, padded to
    the longest, go through ONE MelNet call with row lengths (a row is the mel of that clip alone), the ground-truth accompaniments of the
    items that have them through a second, one mel_distance call scores the mels against the decoded ones (offset removed) and one
    against the ground truth, and one host copy brings the numbers back.  The rows join mel_rows in the order they were queued."""
    from versband_amd.melnet import mel_distance
    for at in range(0, len(pending), 64):
        part = pending[at:at + 64]
        wavs, wav_lens = _padded_rows([w for _, w, _, _ in part], device)
        back = mel_net(wavs, lengths=wav_lens)
        back_frames = [mel_net.frames(n) for n in wav_lens]
        specs, spec_frames = _padded_rows([s for _, _, s, _ in part], device)
        results = [mel_distance(back, specs, [min(a, b) for a, b in zip(back_frames, spec_frames)], remove_offset=True)[0]]
        with_gt = [r for r, (_, _, _, gt) in enumerate(part) if gt is not None]
        if with_gt:
            gts, gt_lens = _padded_rows([part[r][3] for r in with_gt], device)
            ref = mel_net(gts, lengths=gt_lens)
            frames = [min(back_frames[r], mel_net.frames(n)) for r, n in zip(with_gt, gt_lens)]
            results.append(mel_distance(back[with_gt].contiguous(), ref, frames, remove_offset=False)[0])
        values = torch.cat(results).cpu().tolist()                   # the one device-to-host copy of the pass
        for r, (row, _, _, _) in enumerate(part):
            row["mel_l1_vs_decoded"] = values[r]
            if r in with_gt:
                row["mel_l1_vs_gt_accomp"] = values[len(part) + with_gt.index(r)]
            mel_rows.append(row)


@torch.no_grad()
def gen_song(rank, args):
    """gen_song of scripts/test_final.py, group by group: form a group, sample it, write its files, drop it"""
    device = torch.device("cuda:0" if vdist.one_device() else f"cuda:{int(rank)}")
    torch.cuda.set_device(device)
    vdist.init(rank, args.num_gpus, device, master_port=args.master_port)
    dataset = SyntheticDataset(args.synthetic, args.synthetic_frames, args.seed) if args.synthetic else \
        InferDataset(args.manifest_path, args.other_condition, seed=args.seed)
    if rank == 0 and not args.synthetic:
        print("note: 'Musical:' caption sentences come from versband_amd.harness.CaptionGenerator2 - same facts, NOT the reference's wording (see --help)")
    indices = vdist.shard_indices(len(dataset), rank, args.num_gpus)
    sampler = loop.initialize_model(args, device, rank)
    vocoder = loop.make_vocoder(args, device, os.path.join(args.save_dir, f".synthetic_vocoder_{rank}"), rank)
    mel_net = None
    if args.eval_mel:
        from preprocess.NAT_mel import MelNet
        mel_net = MelNet(loop.MEL_HPARAMS, device=device)
    scales = _scales(args)
    rows, mel_rows = [], []
    item_idx = 0
    loaded = ((gi, dataset[gi]) for gi in indices)                  # lazily, in shard order: an item is read when its group is formed
    for group in stream_length_groups(loaded, lambda e: int(e[1]["acoustic"].shape[1] / MEL_DOWNSAMPLE), args.items_per_batch, args.length_slack):
        generated = sample_group(args, sampler, vocoder, group, scales, device)
        pending = []
        for p, (gi, item) in enumerate(group):
            write_item(args, rank, item_idx, item, scales, {s: generated[(p, s)] for s in scales}, rows, pending, mel_net)
            item_idx += 1
        if pending:
            score_group(pending, mel_net, mel_rows, device)           # (one path at every --items_per_batch, 1 included)
        del generated, pending                                               # the group's conditioning, start noise, mels and wavs end here
    tag = "" if args.num_gpus == 1 else f".{rank}"
    csv_path = os.path.join(args.save_dir, f"clap{tag}.csv")
    save_rows_to_tsv(rows, ["audio_path", "caption", "name"], csv_path)
    if mel_rows:
        save_rows_to_tsv(mel_rows, ["name", "scale", "sample", "mel_l1_vs_decoded", "mel_l1_vs_gt_accomp"],
                         os.path.join(args.save_dir, f"mel_l1{tag}.tsv"))
    print(f"[rank {rank}] wrote {len(rows)} generated clips, {csv_path}")
    if args.num_gpus > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    args = parse_args()
    if args.num_gpus > 1:
        import torch.multiprocessing as mp
        mp.spawn(gen_song, nprocs=args.num_gpus, args=(args,))
    else:
        gen_song(0, args=args)
