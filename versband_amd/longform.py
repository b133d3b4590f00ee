"""Long-form generation (BASELINE config 5: 120 s accompaniment) - build-defined, the reference has none.

The reference cannot go past max_len = 1500 latent tokens (40 s): its RoPE table asserts
(vocal2music_moe.py:421, flag_large_dit_moe.py:232) and no chunking exists anywhere in the tree
(SURVEY Q14).  Here a long clip is cut into windows of <= max_len latent tokens that overlap by
`overlap` tokens; every window is an independent "clip" for the sampler (own slice of the midi/beats
tracks, same caption, own slice of the start noise), so all windows of all clips run as ONE batch
through vb_sample_cfg.  Window latents are cross-faded linearly over the overlaps.
(sample_long(mode="continue") gives up that batching for coherence: the windows of a clip are sampled in order and each holds its
overlap with the previous one on the model's probability path - vb_sample_cfg_keep - so the new tokens are generated in agreement with
the music that is already there, and the windows are stitched without a cross-fade.  sample_long(mode="joint") keeps the one batched
call AND is coherent: after every Euler step the overlapping tokens of neighbouring windows are reconciled to one consensus value -
vb_sample_cfg_windows - so every window sees in its overlap the state its neighbour sees, the windows agree bit for bit where they
overlap, and the stitch is plain slicing.)  The VAE decoder is
applied to the whole latent (it is length-agnostic), the HiFi-GAN - fully convolutional - is run in
chunks with a halo larger than its receptive field and the chunks are stitched (overlap-discard), which
reproduces whole-clip vocoding exactly.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

Tensor = torch.Tensor


def plan_windows(T: int, window: int, overlap: int) -> List[Tuple[int, int]]:
    """[(start, length)] covering [0,T) with windows of `window` tokens overlapping by `overlap`."""
    if T <= window:
        return [(0, T)]
    assert 0 <= overlap < window
    hop = window - overlap
    out, s = [], 0
    while True:
        if s + window >= T:
            out.append((T - window, window))
            break
        out.append((s, window))
        s += hop
    return out


def plan_window_rows(lengths: Sequence[int], window: int, overlap: int) -> Tuple[List[int], List[int], List[int]]:
    """(group, start, row_len) of a joint call over clips of different lengths (engine.sample_cfg(window_rows=(group, start),
    lengths=row_len)): plan_windows(T_b, window, overlap) of every clip, concatenated clip by clip - row r is the window of clip group[r]
    over its tokens [start[r], start[r] + row_len[r]).  A clip with T_b <= window is one row of its own length."""
    group, start, row_len = [], [], []
    for b, T_b in enumerate(lengths):
        for s, n in plan_windows(int(T_b), window, overlap):
            group.append(b)
            start.append(s)
            row_len.append(n)
    return group, start, row_len


def crossfade_windows_hip(lib, zw: Tensor, plan: Sequence[Tuple[int, int]], B: int, T: int) -> Tensor:
    """the product path of crossfade_windows: window results zw [nw*B, C, n] (row = w*B + b) -> [B, C, T] by vb_crossfade_windows (one kernel,
    same window order and arithmetic as the torch restatement below, which the oracle fixtures were generated with)"""
    import ctypes as C
    from . import _lib as L
    nw, n = len(plan), plan[0][1]
    assert all(m == n for _, m in plan) and zw.shape[0] == nw * B and zw.shape[2] == n
    zw = zw.contiguous()
    out = torch.empty(B, zw.shape[1], T, dtype=torch.float32, device=zw.device)
    starts = (C.c_int32 * nw)(*[s for s, _ in plan])
    L.check(lib.vb_crossfade_windows(L.ptr(zw), starts, nw, B, zw.shape[1], n, T, L.ptr(out), L.stream_ptr()), "vb_crossfade_windows")
    return out


def crossfade_windows(parts: Sequence[Tensor], plan: Sequence[Tuple[int, int]], T: int) -> Tensor:
    """Blend window results [B,C,len] into [B,C,T]: linear ramps over every overlap, weights sum to one.  (Torch restatement: the CPU
    oracle's digest generator uses it - oracle/gen_bench_digest.py --long; the product path is crossfade_windows_hip.)"""
    B, C = parts[0].shape[:2]
    acc = torch.zeros(B, C, T, dtype=parts[0].dtype, device=parts[0].device)
    wsum = torch.zeros(T, dtype=parts[0].dtype, device=parts[0].device)
    for i, ((s, n), p) in enumerate(zip(plan, parts)):
        w = torch.ones(n, dtype=p.dtype, device=p.device)
        if i > 0:
            ov = plan[i - 1][0] + plan[i - 1][1] - s
            if ov > 0:
                w[:ov] = torch.linspace(0, 1, ov + 2, dtype=p.dtype, device=p.device)[1:-1]
        if i + 1 < len(plan):
            ov = s + n - plan[i + 1][0]
            if ov > 0:
                w[n - ov:] = torch.minimum(w[n - ov:], torch.linspace(1, 0, ov + 2, dtype=p.dtype, device=p.device)[1:-1])
        acc[:, :, s:s + n] += p * w
        wsum[s:s + n] += w
    return acc / wsum


def plan_continue(plan: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int]]:
    """[(start, length, known)] of mode="continue": window w holds its first `known` tokens - its whole overlap with window w - 1, which
    for the last window of plan_windows may be more than `overlap` - and contributes [start + known, start + length) to the result, so
    the contributions cover [0, T) exactly once."""
    out, end = [], 0
    for s, n in plan:
        assert s <= end, "windows must not leave a gap"
        out.append((s, n, end - s))
        end = s + n
    return out


def _checked_lengths(caller: str, lengths, B: int, T: int, rows: str) -> List[int]:
    """the `lengths` argument of sample_long / vocode_chunked / render_long as a list of B integers in [1, T] (rows: what the caller's
    message calls the B entries)"""
    lengths = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lengths) != B:
        raise ValueError(f"{caller}: lengths has {len(lengths)} entries for {B} {rows}")
    for b, n in enumerate(lengths):
        if not 1 <= n <= T:
            raise ValueError(f"{caller}: lengths[{b}] = {n} is not in [1, T = {T}]")
    return lengths


def sample_long(engine, x0: Tensor, t5_cond: Tensor, t5_uncond: Tensor, midi: Tensor, beats: Tensor, t_idx_table, dt_table,
                scale: float, window: int = 1500, overlap: int = 128, seed: int = 0, clip_base: int = 0, mode: str = "crossfade",
                t_next=None, sigma_min: float = 1e-4, return_windows: bool = False, guidance=None, lengths=None):
    """x0 [B,C,T], t5_* [B,L,1024], midi/beats [B,1,2T] -> z [B,C,T] for T beyond the DiT's max_len.
    mode "crossfade" (default): all windows as one batch of independent clips, latents cross-faded over the overlaps.
    mode "continue": windows in order, each with its overlap held on the probability path of the previous window's result (needs
    t_next = model.euler_times of the same grid as the step tables, and the model's sigma_min); no cross-fade.
    mode "joint": all windows as one batch, like "crossfade", with the overlapping tokens of neighbouring windows reconciled to one
    consensus value after every step (engine.sample_cfg(windows=...)); the windows agree bit for bit in their overlaps, no cross-fade.
    (A plan whose shifted last window starts before the end of the window two before it puts a token under three windows and is
    refused by the engine's validation.)
    guidance: per-step guidance weights, handed to every sampler call of the mode (engine.sample_cfg(guidance=...)).
    return_windows (continue and joint modes) also returns every window's full result, overlaps included: (z, [z_w [B,C,n]]).
    lengths (mode "joint" only): B clip lengths T_b <= T in latent tokens - long clips of DIFFERENT lengths in one call.  x0 is [B,C,T]
    and midi / beats hold exactly 2T frames, T the padded length; what lies behind a clip's end is never read.  Every clip gets its own
    plan_windows(T_b, window, overlap) (plan_window_rows), all windows of all clips are rows of one sampler call
    (engine.sample_cfg(window_rows=, lengths=)), and the result is [B,C,T] with zeros behind each clip's end.  Clip b equals
    sample_long on x0[b:b+1, :, :T_b] alone with clip_base + b, bit for bit: its window w draws its router noise under the key it has
    there, (clip_base + b) * nw_b + w with nw_b the clip's window count.  (Keys of different clips can coincide - clip 0's window 2 of
    3 and clip 1's window 0 of 2 at clip_base 0 - exactly as they do across separate calls today.)  return_windows then gives
    (z, [[z_w [1,C,n_w]] per clip]).  None, or all lengths equal to T, is the call without lengths."""
    if mode not in ("crossfade", "continue", "joint"):
        raise ValueError(f"sample_long: mode {mode!r} (crossfade | continue | joint)")
    gk = {} if guidance is None else {"guidance": guidance}        # (None: the calls are the ones they were)
    B, C, T = x0.shape
    window = min(window, engine.cfg.max_len)
    if lengths is not None:
        if mode != "joint":
            raise ValueError(f"sample_long: lengths belong to mode=\"joint\" (mode {mode!r} takes clips of one length)")
        lengths = _checked_lengths("sample_long", lengths, B, T, "clips")
        if any(T_b != T for T_b in lengths):
            return _sample_joint_lengths(engine, x0, t5_cond, t5_uncond, midi, beats, t_idx_table, dt_table, scale, window, overlap, seed,
                                         clip_base, return_windows, guidance, lengths)
    plan = plan_windows(T, window, overlap)
    nw = len(plan)
    n = plan[0][1]
    midi, beats = midi.reshape(B, -1), beats.reshape(B, -1)
    if midi.shape[1] != beats.shape[1] or abs(midi.shape[1] - 2 * T) > 4:
        raise ValueError(f"midi/beats tracks of {midi.shape[1]} / {beats.shape[1]} frames do not match 2 x {T} latent frames")
    if midi.shape[1] < 2 * T:         # a slightly shorter track: repeat the last frame, as the stem does for |T - T_mel/2| <= 2
        pad = 2 * T - midi.shape[1]
        midi = torch.cat([midi, midi[:, -1:].expand(B, pad)], dim=1)
        beats = torch.cat([beats, beats[:, -1:].expand(B, pad)], dim=1)
    if return_windows and mode == "crossfade":
        raise ValueError("sample_long: return_windows belongs to mode=\"continue\" and mode=\"joint\"")
    if mode == "continue":
        if t_next is None:
            raise ValueError('sample_long(mode="continue") needs t_next (model.euler_times of the step tables\' grid)')
        return _sample_continue(engine, x0, t5_cond, t5_uncond, midi, beats, t_idx_table, dt_table, scale, plan, seed, clip_base, t_next,
                                sigma_min, return_windows, guidance)
    # windows become extra batch rows: row = w * B + b
    xw = torch.cat([x0[:, :, s:s + n] for s, _ in plan], dim=0)
    mw = torch.cat([midi[:, 2 * s:2 * (s + n)] for s, _ in plan], dim=0)
    bw = torch.cat([beats[:, 2 * s:2 * (s + n)] for s, _ in plan], dim=0)
    t5 = torch.cat([t5_cond.repeat(nw, 1, 1), t5_uncond.repeat(nw, 1, 1)], dim=0)
    cond = engine.precompute_cond(t5, mw, bw, n, persistent=True)
    if mode == "joint":
        if nw == 1:           # T <= window: the plain call
            zw = engine.sample_cfg(xw, cond, t_idx_table, dt_table, scale, seed=seed, clip_base=clip_base * nw, **gk)
            return (zw, [zw]) if return_windows else zw
        zw = engine.sample_cfg(xw, cond, t_idx_table, dt_table, scale, seed=seed, clip_base=clip_base * nw, windows=[s for s, _ in plan], **gk)
        parts = [zw[w * B:(w + 1) * B] for w in range(nw)]
        # every token from exactly one window (plan_continue); the overlaps hold the same bits in both, so there is nothing to fade
        out = torch.empty(B, C, T, dtype=zw.dtype, device=zw.device)
        for (s, m, known), p in zip(plan_continue(plan), parts):
            out[:, :, s + known:s + m] = p[:, :, known:]
        return (out, parts) if return_windows else out
    zw = engine.sample_cfg(xw, cond, t_idx_table, dt_table, scale, seed=seed, clip_base=clip_base * nw, **gk)
    if nw == 1:
        return zw
    if zw.is_cuda and all(m == n for _, m in plan):
        return crossfade_windows_hip(engine.ctx.lib, zw, plan, B, T)
    parts = [zw[i * B:(i + 1) * B] for i in range(nw)]
    return crossfade_windows(parts, plan, T)


def _sample_joint_lengths(engine, x0, t5_cond, t5_uncond, midi, beats, t_idx_table, dt_table, scale, window, overlap, seed, clip_base,
                          return_windows, guidance, lengths):
    """mode="joint" of sample_long with clip lengths: every window of every clip as a row of its own length in one sampler call, the rows
    of a clip reconciled in their overlaps after every step (vb_window_rows), stitched by plain slicing."""
    B, C, T = x0.shape
    midi, beats = midi.reshape(B, -1), beats.reshape(B, -1)
    if midi.shape[1] != 2 * T or beats.shape[1] != 2 * T:
        raise ValueError(f"sample_long: with lengths, midi / beats hold exactly 2 x {T} frames, got {midi.shape[1]} / {beats.shape[1]}")
    group, start, row_len = plan_window_rows(lengths, window, overlap)
    R, n = len(group), max(row_len)

    def rows(src, mul):
        """the rows cut out of src [B, ..., mul * T] and padded with zeros to mul * n"""
        out = torch.zeros(R, *src.shape[1:-1], mul * n, dtype=src.dtype, device=src.device)
        for r, (b, s, m) in enumerate(zip(group, start, row_len)):
            out[r, ..., :mul * m] = src[b, ..., mul * s:mul * (s + m)]
        return out

    xw, mw, bw = rows(x0, 1), rows(midi, 2), rows(beats, 2)
    t5 = torch.cat([t5_cond[group], t5_uncond[group]], dim=0)
    nw_of = [group.count(b) for b in range(B)]
    first = [group.index(b) for b in range(B)]
    keys = [(clip_base + b) * nw_of[b] + (r - first[b]) for r, b in enumerate(group)]       # the key of window w of clip b sampled alone
    cond = engine.precompute_cond(t5, mw, bw, n, persistent=True, lengths=row_len)
    zw = engine.sample_cfg(xw, cond, t_idx_table, dt_table, scale, seed=seed, clip_ids=keys, window_rows=(group, start), lengths=row_len,
                           guidance=guidance)
    out = torch.zeros(B, C, T, dtype=zw.dtype, device=zw.device)
    parts = [[] for _ in range(B)]
    for b in range(B):
        plan = [(start[r], row_len[r]) for r in range(first[b], first[b] + nw_of[b])]
        for w, (s, m, known) in enumerate(plan_continue(plan)):
            p = zw[first[b] + w:first[b] + w + 1, :, :m]
            out[b:b + 1, :, s + known:s + m] = p[:, :, known:]
            parts[b].append(p)
    return (out, parts) if return_windows else out


def _sample_continue(engine, x0, t5_cond, t5_uncond, midi, beats, t_idx_table, dt_table, scale, plan, seed, clip_base, t_next, sigma_min,
                     return_windows=False, guidance=None):
    """mode="continue" of sample_long: one sampler call of B rows per window.  Window w's noise key is the one it has as rows
    [w*B, (w+1)*B) of the cross-fade batch, so window 0 equals today's window 0."""
    gk = {} if guidance is None else {"guidance": guidance}
    B, C, T = x0.shape
    nw = len(plan)
    dev = engine.ctx.device
    out = torch.empty(B, C, T, dtype=torch.float32, device=dev)
    t5 = torch.cat([t5_cond, t5_uncond], dim=0)
    # one set of known-region buffers per window length: stable addresses let the later windows replay the captured step loop
    bufs, parts = {}, []
    for w, (s, n, known) in enumerate(plan_continue(plan)):
        xw = x0[:, :, s:s + n].to(dev, torch.float32).contiguous()
        cond = engine.precompute_cond(t5, midi[:, 2 * s:2 * (s + n)].contiguous(), beats[:, 2 * s:2 * (s + n)].contiguous(), n, persistent=True)
        keep = None
        if known > 0:
            if n not in bufs:
                bufs[n] = tuple(torch.zeros(shape, dtype=torch.float32, device=dev) for shape in ((B, C, n), (B, C, n), (B, n)))
            ref, xn, mask = bufs[n]
            ref.zero_()
            ref[:, :, :known] = out[:, :, s:s + known]
            xn.copy_(xw)
            mask.zero_()
            mask[:, :known] = 1.0
            keep = (ref, xn, mask, t_next, sigma_min)
        zw = engine.sample_cfg(xw, cond, t_idx_table, dt_table, scale, seed=seed, clip_base=clip_base * nw + w * B, keep=keep, **gk)
        out[:, :, s + known:s + n] = zw[:, :, known:]
        if return_windows:
            parts.append(zw)
    return (out, parts) if return_windows else out


def vocode_chunked(vocoder_net, mel: Tensor, chunk: int = 2048, halo: int = 32, lengths=None) -> Tensor:
    """mel [B,80,T] -> wav [B,1,T*hop] in chunks of `chunk` frames with `halo` frames of context on both sides;
    identical to whole-clip vocoding when halo >= the generator's receptive field (in frames).
    lengths: B mel lengths <= T - long mels of DIFFERENT lengths padded to T in one call (ConvNet.run_chunked(lengths=),
    vb_hifigan_forward_chunked_lens).  Row b holds lengths[b] * hop samples - the chunk loop over that clip alone on the same grid
    (harness.plan_chunk_calls) - followed by zeros; a row that ended before a chunk is not run in it and the mel padding is never read.
    None, or every row full, is the call without lengths."""
    B, _, T = mel.shape
    hop = vocoder_net.out_tmul
    if lengths is not None:
        lengths = _checked_lengths("vocode_chunked", lengths, B, T, "rows")
        if all(n == T for n in lengths):
            lengths = None
    if lengths is not None:
        if hasattr(vocoder_net, "run_chunked"):
            return vocoder_net.run_chunked(mel, chunk, halo, lengths=lengths)
        if T <= chunk + 2 * halo:
            return vocoder_net.run(mel, lengths=lengths)
        # the torch restatement of the plan: per chunk the rows that reach into it, masked at their own ends, through the lengths call
        from . import harness
        out = torch.zeros(B, vocoder_net.out_ch, T * hop, dtype=torch.float32, device=mel.device)
        for c in harness.plan_chunk_calls(lengths, T, chunk, halo):
            if not c["rows"]:
                continue
            x = torch.zeros(len(c["rows"]), mel.shape[1], c["tc"], dtype=mel.dtype, device=mel.device)
            for j, (b, n) in enumerate(zip(c["rows"], c["n"])):
                x[j, :, :n] = mel[b, :, c["lo"]:c["lo"] + n]
            w = vocoder_net.run(x, **({} if all(n == c["tc"] for n in c["n"]) else {"lengths": c["n"]}))
            for j, b in enumerate(c["rows"]):
                e = min(c["e"], lengths[b])
                out[b, :, c["s"] * hop:e * hop] = w[j, :, (c["s"] - c["lo"]) * hop:(e - c["lo"]) * hop]
        return out
    if T <= chunk + 2 * halo:
        return vocoder_net.run(mel)
    if hasattr(vocoder_net, "run_chunked"):
        return vocoder_net.run_chunked(mel, chunk, halo)      # the product path: loop, slicing and stitching inside the library
    out = torch.empty(B, vocoder_net.out_ch, T * hop, dtype=torch.float32, device=mel.device)
    s = 0
    while s < T:
        e = min(T, s + chunk)
        lo, hi = max(0, s - halo), min(T, e + halo)
        w = vocoder_net.run(mel[:, :, lo:hi].contiguous())
        out[:, :, s * hop:e * hop] = w[:, :, (s - lo) * hop:(e - lo) * hop]
        s = e
    return out


def render_long(vae_net, vocoder_net, z: Tensor, lengths=None, chunk: int = 3000, halo: int = 32):
    """latents z [B,zc,T] of B long clips -> their waveforms: the VAE decode and the chunked vocoder, both with row lengths.
    lengths: B latent lengths <= T (tokens).  The rows are decoded in one call per residue of the latent length mod 4
    (harness.plan_decode_calls, ConvNet.decode_lens) and each residue group of the mel lengths (harness.plan_vocoder_calls) is vocoded
    through the chunked lengths call (vocode_chunked(lengths=)); returns a list of B waveforms [out_ch, mel frames * hop] cut to their
    own lengths, each the decode + chunk loop on that clip alone (bit for bit when chunk and halo are multiples of 4: the members of a
    group share their residue, hence so do a row's frames and the width of every chunk).  None: decode + vocode_chunked of the whole
    batch, returned as one tensor [B, out_ch, mel frames * hop] as today."""
    from . import harness
    if lengths is None:
        return vocode_chunked(vocoder_net, vae_net.run(z), chunk, halo)
    B, _, T = z.shape
    lengths = _checked_lengths("render_long", lengths, B, T, "clips")
    up, hop = vae_net.out_tmul, vocoder_net.out_tmul
    mels = [None] * B
    for c in harness.plan_decode_calls(lengths):
        zz = z[c["rows"], :, :c["length"]].contiguous()
        mel = vae_net.run(zz) if c["lengths"] is None else vae_net.decode_lens(zz, c["lengths"])
        for j, b in enumerate(c["rows"]):
            mels[b] = mel[j, :, :lengths[b] * up]
    out = [None] * B
    for c in harness.plan_vocoder_calls([lengths[b] * up for b in range(B)]):
        x = torch.zeros(len(c["rows"]), mels[0].shape[0], c["length"], dtype=torch.float32, device=mels[0].device)
        for j, b in enumerate(c["rows"]):
            x[j, :, :mels[b].shape[1]] = mels[b]
        wav = vocode_chunked(vocoder_net, x, chunk, halo, lengths=c["lengths"])
        for j, b in enumerate(c["rows"]):
            out[b] = wav[j, :, :lengths[b] * up * hop]
    return out
