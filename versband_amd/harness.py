"""Host-side harness I/O of the inference entry point: manifest / condition loading, item assembly, caption text,
wav reading and writing.  Pure plumbing - no GPU work; the behaviour follows scripts/test_final.py:100-347 and :424-463 of the
reference, with its crashes repaired where the intent is unambiguous (each noted at the spot).
"""
from __future__ import annotations

import ast
import csv
import math
import os
import random
import wave
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

MEL_NUM = 80                    # test_final.py:208
MEL_DOWNSAMPLE = 2              # :209  latent length = int(T_mel / 2)
MIN_BATCH_LEN = 75              # :211
PAD_VALUE = -5                  # :212  log-mel floor
UNIT_FRAMES_MULTIPLE = 8        # :214  2 * min_factor
MAX_ITEMS = 200                 # :229  the reference draws 200 random item names
MAX_DURATION = 20.0             # :236


def pad_or_cut_xd(x, length: int, dim: int = 1, pad_value=0):
    """The helper test_final.py:27 imports from ldm/data/joinaudiodataset_anylen.py but the reference never defines:
    cut `x` to `length` along `dim` or pad it with `pad_value`.  numpy in -> numpy out, tensor in -> tensor out."""
    is_t = torch.is_tensor(x)
    a = x.numpy() if is_t else np.asarray(x)
    n = a.shape[dim]
    if n >= length:
        a = np.take(a, np.arange(length), axis=dim)
    else:
        pad = [(0, 0)] * a.ndim
        pad[dim] = (0, length - n)
        a = np.pad(a, pad, constant_values=pad_value)
    return torch.from_numpy(np.ascontiguousarray(a)) if is_t else a


def safe_path(path):
    """`path`, with its directory created if it does not exist yet (the reference's helper of the same name, test_final.py:112-114)"""
    parent = os.path.dirname(os.path.abspath(str(path)))
    os.makedirs(parent, exist_ok=True)
    return path


def load_samples_from_tsv(tsv_path) -> List[Dict[str, str]]:
    """Manifest reader with the reference's contract (test_final.py:116-133): a header row, TAB-separated fields taken literally (no
    quoting rules), one dict per data row; a missing file is an error, an empty manifest only a warning.  Parsed by hand: the fields
    carry no quoting, so splitting the lines is the whole format."""
    if not os.path.isfile(str(tsv_path)):
        raise FileNotFoundError(f"Dataset not found: {tsv_path}")
    with open(str(tsv_path), encoding="utf-8", newline="") as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    lines = [ln for ln in lines if ln != ""]
    if not lines:
        print(f"warning: empty manifest: {tsv_path}")
        return []
    header = lines[0].split("\t")
    samples = []
    for ln in lines[1:]:
        cells = ln.split("\t")
        row = {k: (cells[i] if i < len(cells) else None) for i, k in enumerate(header)}
        if len(cells) > len(header):            # csv.DictReader keeps surplus cells under the key None: same here
            row[None] = cells[len(header):]
        samples.append(row)
    if not samples:
        print(f"warning: empty manifest: {tsv_path}")
    return samples


def save_rows_to_tsv(rows: List[Dict[str, str]], fieldnames: List[str], path) -> None:
    """save_df_to_tsv (test_final.py:100-110) without pandas: header, TAB separated, no quoting, backslash escapes."""
    with open(safe_path(str(path)), "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=fieldnames, delimiter="\t", quoting=csv.QUOTE_NONE, escapechar="\\", lineterminator="\n")
        w.writeheader()
        w.writerows(rows)


# ------------------------------------------------------------------------------------------------------------------
# wav files
# ------------------------------------------------------------------------------------------------------------------
def read_wav(path):
    """soundfile.read(path) -> (float64 samples in [-1, 1), sample rate); falls back to the standard library / scipy when
    soundfile is not installed (this image).  Multi-channel files keep their [n, ch] shape like soundfile."""
    try:
        import soundfile as sf
        return sf.read(path)
    except ImportError:
        pass
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype == np.int16:
        data = data.astype(np.float64) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float64) / 2147483648.0
    elif data.dtype == np.uint8:
        data = (data.astype(np.float64) - 128.0) / 128.0
    else:
        data = data.astype(np.float64)
    return data, sr


def write_wav_pcm16(path, wav, sr: int) -> None:
    """soundfile.write(path, wav, sr, subtype='PCM_16') (test_final.py:433): clip to [-1, 1), scale by 2^15, round-to-nearest."""
    wav = np.asarray(wav, dtype=np.float64)
    try:
        import soundfile as sf
        sf.write(safe_path(path), wav, sr, subtype="PCM_16")
        return
    except ImportError:
        pass
    pcm = np.clip(np.rint(wav * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(safe_path(path), "wb") as f:
        f.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


# ------------------------------------------------------------------------------------------------------------------
# batching of the inference loop (scripts/infer_batched.py --items_per_batch)
# ------------------------------------------------------------------------------------------------------------------
MAX_ROWS_PER_CALL = 32          # rows of one batched sampler call (--items_per_batch is checked against it)


def parse_frames(text) -> List[int]:
    """--synthetic_frames: one integer (every item has that many mel frames, as always) or a comma list that cycles over the items"""
    try:
        frames = [int(v) for v in str(text).split(",")]
    except ValueError:
        raise ValueError(f"--synthetic_frames: expected an integer or a comma list of integers, got {text!r}") from None
    if not frames or any(f < 1 for f in frames):
        raise ValueError(f"--synthetic_frames: frame counts must be positive, got {text!r}")
    return frames


def check_items_per_batch(items_per_batch: int, scales, n_samples: int) -> None:
    """the largest call of plan_row_batches must stay within MAX_ROWS_PER_CALL rows"""
    guided = [s for s in scales if s != 1.0]
    rows = items_per_batch * max(len(guided), 1) * n_samples
    if items_per_batch < 1:
        raise ValueError(f"--items_per_batch must be at least 1, got {items_per_batch}")
    if items_per_batch > 1 and rows > MAX_ROWS_PER_CALL:
        raise ValueError(f"--items_per_batch {items_per_batch} x {max(len(guided), 1)} guided scales x {n_samples} samples = {rows} rows per sampler "
                         f"call; at most {MAX_ROWS_PER_CALL} fit (lower --items_per_batch to {max(1, MAX_ROWS_PER_CALL // (max(len(guided), 1) * n_samples))})")


def stream_groups(items, length_of, items_per_batch: int):
    """the grouping rule, incrementally: consecutive items of equal length, up to items_per_batch of them, as lists in the order given.
    `items` may be a lazy iterable (the CLI loads a manifest item only when its group is formed); length_of(item) is its latent length."""
    group = []
    for it in items:
        if group and (len(group) >= items_per_batch or length_of(it) != length_of(group[0])):
            yield group
            group = []
        group.append(it)
    if group:
        yield group


def stream_length_groups(items, length_of, items_per_batch: int, length_slack: int = 0):
    """stream_groups with a length slack (--length_slack, latent tokens): a consecutive item joins the group while, with it, the longest
    member is at most length_slack tokens longer than EVERY member (max - min <= length_slack) and the group holds fewer than
    items_per_batch items.  Order is preserved; length_slack = 0 is stream_groups, group for group.  A group of mixed lengths is sampled
    as one call padded to its longest member (DiTEngine.sample_cfg(lengths=...))."""
    if length_slack < 0:
        raise ValueError(f"--length_slack must be at least 0, got {length_slack}")
    group, lo, hi = [], 0, 0
    for it in items:
        n = length_of(it)
        if group and (len(group) >= items_per_batch or max(hi, n) - min(lo, n) > length_slack):
            yield group
            group = []
        lo, hi = (min(lo, n), max(hi, n)) if group else (n, n)
        group.append(it)
    if group:
        yield group


def plan_row_batches(lengths, scales, n_samples: int, items_per_batch: int, indices=None, length_slack: int = 0) -> List[dict]:
    """The sampler calls of the inference loop as a list of
        {"n_branch": 1 | 2, "length": latent length, "items": [positions], "rows": [(position, scale, sample)], "clip_ids": [...]}
    lengths[p] is the latent length of the p-th item of this rank's shard, indices[p] its global index (default p); the global clip of a
    row is indices[p] * n_samples + sample, whatever call and slot it rides in.
    Consecutive items (shard order) of equal length form a group of up to items_per_batch items.  Per group there is ONE guided call
    (n_branch = 2; rows = items x scales != 1.0 x samples, item-major, scales in the order given) and, where the scales hold 1.0, one
    unguided call (n_branch = 1; rows = items x samples).  items_per_batch = 1 is the per-item loop as it always ran: one call per
    (item, scale) in the order of `scales`, rows = the item's samples.
    length_slack > 0 groups by stream_length_groups instead; a call over items of different lengths has "length" = its longest item's
    and one more key, "row_lengths": the latent length of every row (the `lengths` of the sampler call).  Calls over equal lengths are
    the dicts they always were."""
    check_items_per_batch(items_per_batch, scales, n_samples)
    lengths = [int(v) for v in lengths]
    indices = list(range(len(lengths))) if indices is None else [int(v) for v in indices]
    if len(indices) != len(lengths):
        raise ValueError(f"plan_row_batches: {len(lengths)} lengths for {len(indices)} indices")

    def call(nb, items, row_scales):
        rows = [(p, s, k) for p in items for s in row_scales for k in range(n_samples)]
        out = {"n_branch": nb, "length": max(lengths[p] for p in items), "items": list(items), "rows": rows,
               "clip_ids": [indices[p] * n_samples + k for p, _, k in rows]}
        if any(lengths[p] != out["length"] for p in items):
            out["row_lengths"] = [lengths[p] for p, _, _ in rows]
        return out

    calls = []
    if items_per_batch == 1:
        for p in range(len(lengths)):
            calls += [call(1 if s == 1.0 else 2, [p], [s]) for s in scales]
        return calls
    guided = [s for s in scales if s != 1.0]
    for items in stream_length_groups(range(len(lengths)), lengths.__getitem__, items_per_batch, length_slack):
        if guided:
            calls.append(call(2, items, guided))
        if len(guided) < len(scales):
            calls.append(call(1, items, [1.0]))
    return calls


def _plan_route_calls(caller: str, row_lengths, mod: int) -> List[dict]:
    """plan_vocoder_calls / plan_decode_calls / plan_encode_calls: one call per residue of the lengths mod `mod`, in the order in which the residues appear"""
    lens = [int(v) for v in row_lengths]
    for r, v in enumerate(lens):
        if v < 1:
            raise ValueError(f"{caller}: row {r} has length {v} (at least 1)")
    groups: Dict[int, List[int]] = {}
    for r, v in enumerate(lens):
        groups.setdefault(v % mod, []).append(r)
    calls = []
    for rows in groups.values():
        member = [lens[r] for r in rows]
        longest = max(member)
        calls.append({"rows": rows, "length": longest, "lengths": member if any(v != longest for v in member) else None})
    return calls


def plan_vocoder_calls(row_lengths_mel) -> List[dict]:
    """The vocoder calls for rows of the given mel lengths (frames), as a list of
        {"rows": [row indices, ascending], "length": the padded length = the longest member, "lengths": [mel length per member] | None}
    Rows whose lengths share a residue mod 4 form one call (HifiGAN.spec2wav_batch(..., lengths=)): the vocoder's kernel routes depend on
    a length only through that residue, so inside such a group every row equals the call on that clip alone bit for bit
    (include/versband_hip.h, vb_hifigan_forward_lens).  At most 4 calls, in the order in which their residues first appear; latent
    lengths make even mel lengths, hence at most 2.  "lengths" is None where the members are all equally long: the plain call."""
    return _plan_route_calls("plan_vocoder_calls", row_lengths_mel, 4)


def plan_chunk_calls(lengths, T: int, chunk: int, halo: int) -> List[dict]:
    """The Python mirror of vb_hifigan_chunked_lens_plan (include/versband_hip.h): the steps of the chunked vocoder over B mels of the
    given lengths (frames) padded to T, as a list of
        {"s", "e", "lo", "tc", "rows": [active rows, ascending], "n": [frames of each active row inside the chunk]}
    The grid is the plain loop's: s = 0, chunk, 2 chunk, ... < T, e = min(s + chunk, T), lo = max(0, s - halo); T <= chunk + 2 halo is one
    step over the whole rows (s = lo = 0, e = T).  A row is active in a step when lengths[b] > s, has n = min(lengths[b], s + chunk + halo)
    - lo frames in it, and keeps the samples of its frames [s, min(e, lengths[b])); tc = the longest n (0 where no row is active).  A
    row equals the chunk loop over the clip alone bit for bit in every step where n % 4 == tc % 4."""
    lens = [int(v) for v in lengths]
    T, chunk, halo = int(T), int(chunk), int(halo)
    if chunk < 1 or halo < 0:
        raise ValueError(f"plan_chunk_calls: chunk = {chunk}, halo = {halo} (chunk >= 1, halo >= 0)")
    if not 1 <= len(lens) <= 64:
        raise ValueError(f"plan_chunk_calls: {len(lens)} rows (1..64)")
    for b, v in enumerate(lens):
        if not 1 <= v <= T:
            raise ValueError(f"plan_chunk_calls: row {b} has length {v} (1..T = {T})")
    whole = T <= chunk + 2 * halo
    steps = []
    for s in ([0] if whole else range(0, T, chunk)):
        e = T if whole else min(s + chunk, T)
        lo = 0 if whole else max(0, s - halo)
        hi = T if whole else s + chunk + halo
        rows = [b for b, v in enumerate(lens) if v > s]
        n = [min(lens[b], hi) - lo for b in rows]
        steps.append({"s": s, "e": e, "lo": lo, "tc": max(n, default=0), "rows": rows, "n": n})
    return steps


DECODE_ROUTE_MOD = 4        # the VAE decoder's bits depend on a latent length through its residue mod 4 alone (include/versband_hip.h, vb_vae_decode_lens)


def plan_decode_calls(row_lengths) -> List[dict]:
    """The VAE decoder's twin of plan_vocoder_calls, for rows of the given latent lengths (tokens): a list of
        {"rows": [row indices, ascending], "length": the padded length = the longest member, "lengths": [latent length per member] | None}
    Rows whose lengths share a residue mod 4 form one call (decode_first_stage(..., lengths=)): a route that changes bits - minimal
    filtering against the direct kernels, the float4 paths of the glue kernels - depends on a length through (length * tmul) % 4 alone;
    what the attention block's two products take from the length (Ci % 16, Co % 4, the rounding of the split planes to 32) chooses
    between bit-identical kernels and adds exact zeros.  Inside such a group every row equals the decode of that clip alone bit for bit.  The calls come in the order in which their residues first appear; "lengths" is None where the members are all
    equally long: the plain call."""
    return _plan_route_calls("plan_decode_calls", row_lengths, DECODE_ROUTE_MOD)


ENCODE_ROUTE_MOD = 4        # the VAE encoder's stages run at tmul = in_tmul .. 1 and (length * tmul) % 4 is a function of length % 4 (include/versband_hip.h, vb_vae_encode_lens)


def plan_encode_calls(row_lengths) -> List[dict]:
    """The VAE encoder's twin of plan_decode_calls, for mels of the given LATENT lengths (tokens; a mel of n frames has n / in_tmul): a list of
        {"rows": [row indices, ascending], "length": the padded length = the longest member, "lengths": [latent length per member] | None}
    Rows whose lengths share a residue mod 4 form one call (encode_first_stage(..., lengths=)).  The predicates of the encoder's routes
    that change bits are the decoder's - minimal filtering against the direct kernels, staged epilogues, the float4 paths of the glue
    kernels - at (length * tmul) % 4; the strided down-convolutions bound their window by the padded row (T_in / 2, no length enters), and
    the attention's channel counts choose between bit-identical kernels and add exact zeros.  Inside such a group every row equals the
    encode of that clip alone bit for bit.  The calls come in the order in which their residues first appear; "lengths" is None where the
    members are all equally long: the plain call."""
    return _plan_route_calls("plan_encode_calls", row_lengths, ENCODE_ROUTE_MOD)


# ------------------------------------------------------------------------------------------------------------------
# caption text (the "Musical: ..." half of the prompt)
# ------------------------------------------------------------------------------------------------------------------
_PITCH_CLASSES = ["C", "C-sharp", "D", "E-flat", "E", "F", "F-sharp", "G", "A-flat", "A", "B-flat", "B"]
_STEP = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}


def _parse_key(key: str):
    """'C major' / 'a minor' / music21-style 'F#' (major), 'b-' (minor: lower case) -> (pitch class, mode)."""
    parts = key.strip().split()
    tonic = parts[0]
    mode = parts[1].lower() if len(parts) > 1 else ("minor" if tonic[0].islower() else "major")
    pc = _STEP[tonic[0].lower()]
    for ch in tonic[1:]:
        pc += 1 if ch == "#" else (-1 if ch in "-b" else 0)
    return pc % 12, mode


class CaptionGenerator2:
    """Drop-in for ldm/modules/encoders/caption_generator.py:781 CaptionGenerator2.transcribe (called at test_final.py:260-268).

    Same inputs, same decision rules - confidence gates 0.5 (key) / 0.3 (tempo) (:63-64); the class boundaries of CaptionGenerator2
    with their deliberate dead zones between classes (tempo 69 / 71-89 / 91-119 / 121-159 / 161, :785-802; average pitch 53 / 56-62 /
    64-77 / 79, :804-819; duration 4.5 / 5.5-9.5 / 10.5-14.5 / 15.5, :821-837, with an even chance of the exact "N seconds"); a
    coin flip to the relative key (:617-618); emotions joined in random order (:659-670).  The SENTENCES are composed here from
    the factors that survive - the reference instead picks from ~25 tables of hand-written English templates, which are prose, not
    behaviour, and are not reproduced: caption strings therefore differ from the reference's while carrying the same facts.
    music21 (absent here) is replaced by pitch-class arithmetic for naming keys."""

    key_min_conf = 0.5
    tempo_min_conf = 0.3
    tempo_words = {"very low": ["very slow"], "low": ["slow", "gentle"], "medium": ["medium", "moderate"], "high": ["fast", "quick"],
                   "very high": ["very fast"]}
    pitch_words = {"low": ["low", "relatively low"], "medium": ["medium", "average"], "high": ["high", "relatively high"],
                   "very high": ["very high"]}
    duration_words = {"short": ["a short time"], "medium": ["a medium stretch of time"], "long": ["a long time"],
                      "very long": ["a very long time"]}

    def __init__(self, rng: Optional[random.Random] = None):
        self.rng = rng or random.Random()

    @staticmethod
    def _classify(v: float, bounds):
        """bounds: [(lo, hi, name)]; values in no interval (the dead zones) give None."""
        for lo, hi, name in bounds:
            if lo <= v < hi:
                return name
        return None

    def prepare_key(self, key, key_conf):
        if key is None or key == "None" or key_conf < self.key_min_conf:
            return None
        pc, mode = _parse_key(str(key))
        if self.rng.random() > 0.5:                               # relative key: same notes, other mode
            pc, mode = ((pc + 9) % 12, "minor") if mode == "major" else ((pc + 3) % 12, "major")
        return f"{_PITCH_CLASSES[pc]} {mode}"

    def prepare_tempo(self, tempo, tempo_conf):
        if tempo is None or tempo <= 0 or tempo_conf < self.tempo_min_conf:
            return None
        c = self._classify(tempo, [(-math.inf, 69, "very low"), (71, 89, "low"), (91, 119, "medium"), (121, 159, "high"),
                                   (161, math.inf, "very high")])
        return self.rng.choice(self.tempo_words[c]) if c else None

    def prepare_avg_pitch(self, avg_pitch):
        if avg_pitch is None or avg_pitch <= 0:
            return None
        c = self._classify(avg_pitch, [(-math.inf, 53, "low"), (56, 62, "medium"), (64, 77, "high"), (79, math.inf, "very high")])
        return self.rng.choice(self.pitch_words[c]) if c else None

    def prepare_emotion(self, emotion):
        if emotion is None or emotion == "None" or len(emotion) == 0:
            return None
        e = list(emotion)
        self.rng.shuffle(e)
        if len(e) <= 2:
            return " and ".join(e)
        return ", ".join(e[:-1]) + ", and " + e[-1]

    def prepare_duration(self, duration):
        if duration is None or duration <= 0:
            return None
        exact = f"{round(duration)} seconds"
        c = self._classify(duration, [(-math.inf, 4.5, "short"), (5.5, 9.5, "medium"), (10.5, 14.5, "long"), (15.5, math.inf, "very long")])
        words = self.rng.choice(self.duration_words[c]) if c else None
        pick = self.rng.choice([words, exact])
        return pick

    def transcribe(self, key=None, key_conf=0.0, avg_pitch=None, tempo=None, tempo_conf=0.0, emotion=None, duration=None) -> str:
        key = self.prepare_key(key, key_conf)
        tempo = self.prepare_tempo(tempo, tempo_conf)
        avg_pitch = self.prepare_avg_pitch(avg_pitch)
        emotion = self.prepare_emotion(emotion)
        duration = self.prepare_duration(duration)
        traits = []
        if key:
            traits.append(f"is in {key}")
        if avg_pitch:
            traits.append(f"sits at a {avg_pitch} pitch")
        if tempo:
            traits.append(f"moves at a {tempo} tempo")
        if duration and traits:
            traits.append(f"lasts {duration}")
        if not traits and not emotion:
            return ""                                             # the reference's `caption = ''` fall-through (:741, :777)
        out = ""
        if traits:
            body = traits[0] if len(traits) == 1 else ", ".join(traits[:-1]) + " and " + traits[-1]
            out = f"The melody {body}."
        if emotion:
            out = (out + " " if out else "") + f"It carries a {emotion} mood."
        return out


# ------------------------------------------------------------------------------------------------------------------
# dataset
# ------------------------------------------------------------------------------------------------------------------
class InferDataset:
    """InferDataset of scripts/test_final.py:196-340.

    manifest (TSV) columns used: name, duration, caption ('<psep>'-separated alternatives), key, key_confidence, avg_pitch, tempo,
    tempo_confidence, emotion (a Python list literal), wav_len, mel_path ([80, T] .npy), vocal_mel_path (.npy, first 20 rows are
    the 'acoustic' condition), audio_path.  `other_condition` is the midi dictionary (.npy holding {name: [T] array}); the beats
    dictionary sits beside it with 'midi' -> 'beats' in the path (:218-226).

    Differences from the reference, all where it cannot run as written: `beats` is read from the beats dictionary (the reference
    only assigns it on its corrupted-input branch and raises NameError otherwise, :282-305); at most - not exactly - 200 items are
    drawn, with a seedable RNG (random.sample(keys, 200) raises on smaller manifests, :229); `eval()` of the emotion column is a
    literal parse."""

    mel_num = MEL_NUM
    mel_downsample_rate = MEL_DOWNSAMPLE
    min_batch_len = MIN_BATCH_LEN
    pad_value = PAD_VALUE
    unit_upsample_rate = 1
    unit_frames_multiple = UNIT_FRAMES_MULTIPLE

    def __init__(self, manifest_path, other_condition, seed: Optional[int] = None, max_items: int = MAX_ITEMS):
        samples = load_samples_from_tsv(manifest_path)
        items_dict = {s["name"]: s for s in samples}
        self.rng = random.Random(seed)
        self.np_rng = np.random.RandomState(seed)
        self.caption_generator = CaptionGenerator2(self.rng)
        self.unit_pad_value = self.pad_value                                      # :216 (the last assignment wins)
        midi_path = str(other_condition)
        beats_path = midi_path.replace("midi", "beats")
        print(f"MIDI path: {midi_path}")
        print(f"Beats path: {beats_path}")
        midi_dict = np.load(midi_path, allow_pickle=True).item()
        beats_dict = np.load(beats_path, allow_pickle=True).item()
        names = list(items_dict.keys())
        self.pred_list = self.rng.sample(names, min(max_items, len(names)))
        self.items = []
        for name in self.pred_list:
            item = items_dict[name]
            if float(item["duration"]) > MAX_DURATION:
                continue
            if name not in midi_dict or name not in beats_dict:
                print(f"no midi / beats for {name}: skipped")
                continue
            item["midi"], item["beats"], item["name"] = midi_dict[name], beats_dict[name], name
            self.items.append(item)

    def __len__(self):
        return len(self.items)

    def _caption(self, data):
        style = self.np_rng.choice(data["caption"].split("<psep>"))
        caption = f"Style: {style} "
        emotion = data.get("emotion", "None")
        try:
            emotion = ast.literal_eval(emotion) if isinstance(emotion, str) else emotion
        except (ValueError, SyntaxError):
            emotion = None
        prompt = self.caption_generator.transcribe(
            key=data.get("key"), key_conf=float(data.get("key_confidence", 0) or 0), avg_pitch=float(data.get("avg_pitch", 0) or 0),
            tempo=float(data.get("tempo", 0) or 0), tempo_conf=float(data.get("tempo_confidence", 0) or 0), emotion=emotion,
            duration=float(data.get("wav_len", 0) or 0))
        return caption, caption + f"Musical: {prompt}"

    def __getitem__(self, index):
        data = self.items[index]
        ori_caption, caption = self._caption(data)
        up = self.unit_upsample_rate
        try:
            spec = np.load(data["mel_path"])                                       # [80, T]
        except Exception:
            print(f"corrupted: {data['mel_path']}")
            spec = np.ones((self.mel_num, self.min_batch_len), dtype=np.float32) * self.pad_value
        org_spec_len = spec_len = spec.shape[1]
        start = 0
        acoustic = np.load(data["vocal_mel_path"])[:20, :]
        midi = np.expand_dims(np.asarray(data["midi"]), axis=0)                    # [1, T]
        beats = np.expand_dims(np.asarray(data["beats"]), axis=0)
        if abs(math.ceil(acoustic.shape[1] * up) - org_spec_len) > 5:              # some bad mel could exist (:282)
            print(f"corrupted: {data['vocal_mel_path']}")
            n = math.ceil(spec_len / up)
            acoustic = np.ones((20, n), dtype=np.float32) * self.unit_pad_value
            midi = np.ones((1, n), dtype=np.float32) * 128
            beats = np.ones((1, n), dtype=np.float32) * 2
        acoustic_len = acoustic.shape[1] + 75                                      # :287
        if math.ceil(acoustic_len * up) > org_spec_len:
            start = round(start * up)
            start = max(min(start, acoustic_len - math.ceil(org_spec_len / up) - 1), 0)
            acoustic_len = math.ceil(org_spec_len / up)
            acoustic = acoustic[:, start:start + acoustic_len]
            midi = midi[:, start:start + acoustic_len]
            beats = beats[:, start:start + acoustic_len]
        acoustic_len = int(math.ceil(acoustic_len / self.unit_frames_multiple) * self.unit_frames_multiple)
        acoustic = pad_or_cut_xd(torch.FloatTensor(np.asarray(acoustic, dtype=np.float32)), acoustic_len, dim=1, pad_value=self.pad_value)
        midi = pad_or_cut_xd(torch.FloatTensor(np.asarray(midi, dtype=np.float32)), acoustic_len, dim=1, pad_value=0)
        beats = pad_or_cut_xd(torch.FloatTensor(np.asarray(beats, dtype=np.float32)), acoustic_len, dim=1, pad_value=0)
        spec_len = math.ceil(acoustic_len * up)
        spec = pad_or_cut_xd(torch.FloatTensor(np.asarray(spec, dtype=np.float32)), spec_len, dim=1, pad_value=self.pad_value)
        assert spec.shape[1] == acoustic.shape[1]
        return {"acoustic": acoustic, "image": spec, "ori_caption": ori_caption, "caption": caption, "name": data["name"], "midi": midi,
                "beats": beats, "audio_path": data.get("audio_path")}

    def collator(self, samples):
        return samples
