"""Python host side over the C ABI: device context, DiT engine, conv-net programs.

torch is used for device memory, streams and checkpoint tensors only; every
compute step of the hot path is a call into libversband_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import pack
from .synth import DiTConfig, HifiGanConfig, VAEConfig

Tensor = torch.Tensor


def _require_gpu(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise L.VersbandError("versband_amd runs on an MI355X only: no HIP device is visible (there is no CPU fallback)")
    return device


class Context:
    """One vb_ctx per (process, device) - mirrors the reference's one process per GPU."""

    def __init__(self, device="cuda:0"):
        self.device = _require_gpu(device)
        self.lib = L.load()
        self.handle = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        torch.cuda.set_device(idx)
        L.check(self.lib.vb_ctx_create(idx, C.byref(self.handle)), "vb_ctx_create")
        self._keep: List[object] = []

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.vb_ctx_destroy(self.handle)
        except Exception:
            pass


# ---------------------------------------------------------------------------
# DiT
# ---------------------------------------------------------------------------


def _ref(struct):
    """an optional ABI struct by reference (None -> NULL), as L.ptr does for tensors"""
    return C.byref(struct) if struct is not None else None


def _device_tables(tables: dict, key: tuple, make) -> tuple:
    """the device copies of one set of step tables ((t_idx, dt) or (t_next,)), made once per distinct key: step tables live on the
    device, so nothing on the host has to outlive the async launch.  The cache is emptied rather than grown past 16 entries."""
    if key not in tables:
        if len(tables) > 16:
            tables.clear()
        tables[key] = make()
    return tables[key]


_KINDS = {"integers": (int, np.integer), "numbers": (int, float, np.integer, np.floating)}


def _checked_list(name: str, v, kind: Optional[str], count: Optional[Tuple[int, str]], what: str, gloss: str = "",
                  count_first: bool = False) -> list:
    """one of the sampler options' sequences - a tensor or any iterable - as a checked Python list.  kind: "integers" / "numbers" (a bool
    is neither; None: the elements are the caller's to convert); count: (n, noun) - n entries, one per "rows" / "steps" (None: any
    number); what / gloss: the caller's wording of the two TypeErrors, "{name} must be {what}, got ..." and "{name} must hold
    {kind}{gloss}".  A wrong element is reported before a wrong count, or after it (count_first)."""
    if torch.is_tensor(v):
        v = v.tolist()
    try:
        vals = list(v)
    except TypeError:
        raise TypeError(f"{name} must be {what}, got {type(v).__name__}") from None
    bad_count = count is not None and len(vals) != count[0]
    bad_kind = kind is not None and any(isinstance(s, bool) or not isinstance(s, _KINDS[kind]) for s in vals)
    if bad_kind and not (count_first and bad_count):
        raise TypeError(f"{name} must hold {kind}{gloss}")
    if bad_count:
        raise ValueError(f"{name} has {len(vals)} entries for {count[0]} {count[1]}")
    return vals


def _lens_struct(lengths, B: int, T: int, windows=None, T_mel: Optional[int] = None, cond: Optional[dict] = None,
                 gloss: str = " (latent tokens per row)"):
    """validate the row lengths of a call - B integers in [1, T], the library's rules (include/versband_hip.h), stated here first so
    that the error names the caller's argument - and lay them out as vb_lens (a host array, read during the call).  All equal to T
    or None is the plain call.  cond: the conditioning handle the call samples from, which must have been made with the same
    lengths.  Returns (struct or None, the array to hold, the lengths as a tuple or None).  Serves the sampler's rows
    (latent tokens) and the vocoder's (ConvNet.run: input frames)."""
    lens = None
    if lengths is not None:
        vals = [int(v) for v in _checked_list("lengths", lengths, "integers", (B, "rows"), f"a sequence of {B} row lengths", gloss)]
        if B > 64:
            raise ValueError(f"lengths: {B} rows (at most 64)")
        for b, v in enumerate(vals):
            if not 1 <= v <= T:
                raise ValueError(f"lengths[{b}] = {v} is not in [1, T = {T}]")
        if any(v != T for v in vals):
            lens = tuple(vals)
    if cond is not None and cond.get("lengths") != lens:
        raise ValueError(f"lengths {lens} differ from the lengths the conditioning was made with ({cond.get('lengths')})")
    if lens is None:
        return None, None, None
    if windows is not None and len(list(windows)) > 1:
        raise ValueError("lengths and joint windows do not go together: windows are equal-length by construction")
    if T_mel is not None and T_mel != 2 * T:
        raise ValueError(f"lengths need midi / beats of exactly 2 * T = {2 * T} frames, got {T_mel}")
    arr = (C.c_int32 * B)(*lens)
    return L.Lens(arr), arr, lens


def _check_device(name: str, t: Tensor, dev):
    """a tensor handed to the engine lives on the host (it is then copied) or on the engine's device"""
    if t.device.type != "cpu" and t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, the engine on {dev}")


class DiTEngine:
    """TxtFlagLargeImprovedDiTV2 (vocal2music_moe.py:477-520) + CFMSampler hot loop on the GPU.

    precision "bf16"  : plain bf16 MFMA operands (production / benchmark)
    precision "split" : bf16x3 split operands (fp32-class, parity tests)"""

    def __init__(self, ctx: Context, cfg: DiTConfig, state_dict: Dict[str, Tensor], precision: str = "bf16", share: "DiTEngine" = None):
        assert precision in ("bf16", "split")
        ctx = Context(ctx.device)        # a vb_ctx holds ONE loaded DiT: every engine owns its handle
        self.ctx, self.cfg, self.precision = ctx, cfg, precision
        self.np = 2 if precision == "split" else 1
        dev = ctx.device
        # engines of one process that serve different sub-batches share ONE packed copy of the weights (`share`)
        # (`share` must be an engine of the SAME configuration, precision and checkpoint: anything else would hand vb_dit_load another
        #  model's pointer layout silently)
        if share is not None:
            if share.cfg != cfg or share.precision != precision:
                raise ValueError(f"DiTEngine(share=...): the shared engine was built for {share.cfg} / {share.precision}, this one asks for {cfg} / {precision}")
            if share._sd_id is not state_dict and share._sd_id is not None and state_dict is not None:
                same = set(share._sd_id.keys()) == set(state_dict.keys()) and all(
                    share._sd_id[k].data_ptr() == state_dict[k].data_ptr() for k in list(state_dict.keys())[:8])
                if not same:
                    raise ValueError("DiTEngine(share=...): the shared engine holds another checkpoint")
        self._sd_id = state_dict
        self.packed = share.packed if share is not None else pack.pack_dit(state_dict, cfg, self.np, dev)
        self.ccfg = L.DitConfig(cfg.in_channels, cfg.hidden_size, cfg.num_heads, cfg.depth, cfg.num_experts, cfg.ffn_hidden,
                                cfg.context_dim, cfg.ori_dim, cfg.max_len, self.np, cfg.norm_eps)
        w = L.DitWeights()
        for name in L.TOP_FIELDS:
            t = self.packed["top"][name]
            setattr(w, name, t.data_ptr() if t is not None else None)
        for i, b in enumerate(self.packed["blocks"]):
            for name in L.BLOCK_FIELDS:
                setattr(w.blocks[i], name, b[name].data_ptr())
        self.cw = w
        L.check(ctx.lib.vb_dit_load(ctx.handle, C.byref(self.ccfg), C.byref(w)), "vb_dit_load")
        self._ws: Optional[Tensor] = None
        self._ws_key = None
        self._checked: Dict[tuple, tuple] = {}                   # range-checked resident index tracks: key -> (midi, beats, versions), references held
        self._tables: Dict[tuple, Tuple[Tensor, Tensor]] = {}    # device copies of the (t_idx, dt) step tables
        self._pcond: Dict[tuple, list] = {}                      # persistent conditioning buffers: key -> [buffer, generation]
        self._xbuf: Dict[tuple, Tensor] = {}                     # engine-owned sampler state (stable address for graph replay)
        self._rowbuf: Dict[tuple, Tensor] = {}                   # staged per-row scales / clip ids: (B, kind) -> device tensor (stable address)

    # -- buffers -----------------------------------------------------------
    def _workspace(self, B, nb, T, Lc) -> Tensor:
        key = (B, nb, T, Lc)
        if self._ws_key != key:
            n = self.ctx.lib.vb_dit_workspace_bytes(C.byref(self.ccfg), B, nb, T, Lc)
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.ctx.device)
            self._ws_key = key
        return self._ws

    # -- API ---------------------------------------------------------------
    def precompute_cond(self, t5: Tensor, midi: Tensor, beats: Tensor, T: int, persistent: bool = False, lengths=None) -> dict:
        """t5 [nb*B, L, ori] (cond rows then uncond rows), midi/beats [B,1,T_mel] or [B,T_mel] int64.
        lengths: B row lengths in latent tokens (vb_lens) - row b's conditioning is that of the clip alone, midi / beats beyond
        2 * lengths[b] are not read; needs T_mel == 2 T.  The handle remembers them: sample_cfg / forward must be given the same.
        persistent=True writes into an engine-owned buffer that the NEXT persistent precompute of the same shape overwrites (a
        serving loop: precompute -> sample -> discard): stable device addresses are what lets sample_cfg replay its captured
        hipGraph.  A stale handle is refused loudly (generation check) instead of sampling from overwritten conditioning."""
        dev = self.ctx.device
        t5 = t5.to(dev, torch.float32).contiguous()
        midi_in, beats_in = midi, beats
        midi = midi.to(dev, torch.int64).reshape(midi.shape[0], -1).contiguous()
        beats = beats.to(dev, torch.int64).reshape(beats.shape[0], -1).contiguous()
        B, T_mel = midi.shape
        Beff, Lc, _ = t5.shape
        nb = Beff // B
        assert nb * B == Beff and nb in (1, 2)
        # range check of the embedding indices (embed_t_kernel reads table[idx * D ..] unclamped): ONE device->host read per new pair
        # of tracks.  The check is skipped only when the CALLER's own tensors are what the kernel will read (resident int64 contiguous
        # device tensors: .to() / reshape / contiguous returned views of the same storage) AND were checked before at the same
        # version; the cache entry holds a reference to them, so their addresses cannot be recycled for other data while the entry
        # lives.  Converted temporaries (CPU, int32, strided inputs) are checked on every call.
        resident = (midi.data_ptr() == midi_in.data_ptr() and beats.data_ptr() == beats_in.data_ptr() and
                    midi_in.dtype == torch.int64 and beats_in.dtype == torch.int64 and midi_in.device == midi.device and
                    beats_in.device == beats.device and midi_in.is_contiguous() and beats_in.is_contiguous())
        key = (midi.data_ptr(), beats.data_ptr(), midi.numel(), beats.numel())
        hit = self._checked.get(key) if resident else None
        # (a view of the same storage shares its version counter, and the held reference keeps that storage - hence the address - alive)
        if hit is None or hit[2] != (midi_in._version, beats_in._version):
            lim = torch.stack([midi.min(), midi.max(), beats.min(), beats.max()]).tolist()
            if lim[0] < 0 or lim[1] >= 130 or lim[2] < 0 or lim[3] >= 3:
                raise IndexError("midi/beats index out of range of the embedding tables (130 / 3 rows)")
            if resident:
                if len(self._checked) > 64:
                    self._checked.clear()
                self._checked[key] = (midi_in, beats_in, (midi_in._version, beats_in._version))
        n = self.ctx.lib.vb_dit_cond_bytes(C.byref(self.ccfg), B, nb, T, Lc)
        gen = None
        if persistent:
            key = (B, nb, T, Lc)
            slot = self._pcond.get(key)
            if slot is None or slot[0].numel() != n:
                slot = [torch.empty(n, dtype=torch.uint8, device=dev), 0]
                self._pcond[key] = slot
            slot[1] += 1
            cond, gen = slot[0], slot[1]
        else:
            cond = torch.empty(n, dtype=torch.uint8, device=dev)
        ws = self._workspace(B, nb, T, Lc)
        ls, held_lens, lens = DiTEngine._lens_struct(lengths, B, T, T_mel=T_mel)
        L.check(self.ctx.lib.vb_dit_precompute_cond_lens(self.ctx.handle, L.ptr(t5), L.ptr(midi), L.ptr(beats), B, nb, T, T_mel, Lc,
                                                         _ref(ls), L.ptr(cond), L.ptr(ws), L.stream_ptr()), "vb_dit_precompute_cond_lens")
        return {"buf": cond, "B": B, "nb": nb, "T": T, "L": Lc, "gen": gen, "lengths": lens}

    def _check_cond(self, cond: dict):
        if cond.get("gen") is not None:
            slot = self._pcond.get((cond["B"], cond["nb"], cond["T"], cond["L"]))
            if slot is None or slot[1] != cond["gen"] or slot[0] is not cond["buf"]:
                raise L.VersbandError("stale persistent conditioning handle: a later precompute_cond(persistent=True) of the same shape "
                                      "overwrote this buffer")

    def _noise_struct(self, noise, seed, clip_base, nfe):
        ns = L.Noise()
        keep = None
        if noise is not None:
            g1, g2, g3 = [t.to(self.ctx.device, torch.float32).contiguous() for t in noise]
            ns.g1, ns.g2, ns.g3 = g1.data_ptr(), g2.data_ptr(), g3.data_ptr()
            keep = (g1, g2, g3)
        ns.seed, ns.clip_base, ns.nfe = seed, clip_base, nfe
        return ns, keep

    def forward(self, x: Tensor, t_idx: Tensor, cond: dict, noise=None, seed: int = 0, clip_base: int = 0, nfe: int = 0,
                return_routes: bool = False, lengths=None):
        """x [B,C,T] f32, t_idx int64 [nb*B]; noise = (g1 [depth,rows,2], g2 [depth,rows,E], g3 [depth,rows,E]) Gumbel
        draws or None -> v [nb*B, C, T] (+ routes int32 [depth,2,rows]).  lengths: the row lengths the conditioning was made with
        (vb_lens); v and the routes of padding tokens are unspecified."""
        dev = self.ctx.device
        B, nb, T, Lc = cond["B"], cond["nb"], cond["T"], cond["L"]
        self._check_cond(cond)
        x = x.to(dev, torch.float32).contiguous()
        t_idx = t_idx.to(dev, torch.int64).contiguous()
        assert x.shape == (B, self.cfg.in_channels, T) and t_idx.numel() == nb * B
        v = torch.empty(nb * B, self.cfg.in_channels, T, dtype=torch.float32, device=dev)
        routes = torch.empty(self.cfg.depth, 2, nb * B * T, dtype=torch.int32, device=dev) if return_routes else None
        ns, keep = self._noise_struct(noise, seed, clip_base, nfe)
        ws = self._workspace(B, nb, T, Lc)
        ls, held_lens, _ = DiTEngine._lens_struct(lengths, B, T, cond=cond)
        L.check(self.ctx.lib.vb_dit_forward_lens(self.ctx.handle, L.ptr(x), L.ptr(t_idx), L.ptr(cond["buf"]), C.byref(ns), B, nb, T, Lc,
                                                 _ref(ls), L.ptr(v), L.ptr(routes), L.ptr(ws), L.stream_ptr()), "vb_dit_forward_lens")
        return (v, routes) if return_routes else v

    def _keep_struct(self, keep, B: int, T: int, n: int):
        """validate a known-region block (ref, x0, mask, t_next, sigma_min) - a tuple or a dict of those names - and lay it out as vb_keep.
        Conforming device tensors are passed as they are (their addresses key the captured graph); returns (struct, references to hold)."""
        dev = self.ctx.device
        names = ("ref", "x0", "mask", "t_next", "sigma_min")
        if isinstance(keep, dict):
            if set(keep) != set(names):
                raise ValueError(f"keep: expected the keys {names}, got {tuple(keep)}")
            keep = tuple(keep[k] for k in names)
        if len(keep) != 5:
            raise ValueError("keep: expected (ref, x0, mask, t_next, sigma_min)")
        ref, x0k, mask, t_next, sigma_min = keep
        shape = (B, self.cfg.in_channels, T)
        for name, t, want in (("ref", ref, shape), ("x0", x0k, shape), ("mask", mask, (B, T))):
            if not torch.is_tensor(t):
                raise TypeError(f"keep: {name} must be a tensor")
            if tuple(t.shape) != want:
                raise ValueError(f"keep: {name} has shape {tuple(t.shape)}, expected {want}")
            if t.dtype != torch.float32:
                raise TypeError(f"keep: {name} must be float32, got {t.dtype}")
            _check_device(f"keep: {name}", t, dev)
        if mask.numel() and (float(mask.min()) < 0.0 or float(mask.max()) > 1.0 or bool(torch.isnan(mask).any())):
            raise ValueError("keep: mask values must lie in [0, 1]")
        t_next = [float(v) for v in _checked_list("keep: t_next", t_next, None, (n, "steps"), f"a sequence of {n} times")]
        ref, x0k, mask = [t.to(dev).contiguous() for t in (ref, x0k, mask)]
        tn, = _device_tables(self._tables, ("t_next", tuple(t_next)), lambda: (torch.tensor(t_next, dtype=torch.float32, device=dev),))
        ks = L.Keep(ref.data_ptr(), x0k.data_ptr(), mask.data_ptr(), tn.data_ptr(), float(sigma_min))
        return ks, (ref, x0k, mask, tn)

    def _rows_struct(self, scale, clip_ids, B: int, clip_base: int = 0):
        """validate per-row guidance scales / global clip ids and lay them out as vb_rows.  A conforming device tensor (float32 / int64,
        [B], contiguous, on the engine's device) is passed as it is - its address keys the captured graph, as with `keep`; host values are
        staged into an engine-owned device buffer reused per (B, kind), so repeated calls replay.  Host values are checked for finiteness;
        a device tensor is not read here (that would be a device-to-host sync in front of every replay): its contents are the caller's
        contract.  A plain number as `scale` is today's scalar path (no array).  Returns (struct or None, scalar scale, references to hold)."""
        dev = self.ctx.device
        held = []

        def rows(name, v, dtype, kind):
            if torch.is_tensor(v):
                if v.dtype != dtype:
                    raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {str(v.dtype).replace('torch.', '')}")
                if v.dim() != 1 or v.numel() != B:
                    raise ValueError(f"{name} has shape {tuple(v.shape)}, expected ({B},)")
                _check_device(name, v, dev)
                if v.device == dev and v.is_contiguous():       # (not read here: no device-to-host sync on the replay path)
                    held.append(v)
                    return v
                if kind == "scale" and v.device.type == "cpu" and not bool(torch.isfinite(v).all()):
                    raise ValueError(f"{name} must be finite")
                vals = v
            else:
                what = "a number, a sequence or a float32 tensor" if kind == "scale" else "a sequence or an int64 tensor"
                vals = _checked_list(name, v, "numbers" if kind == "scale" else "integers", (B, "rows"), f"{what} of {B} values",
                                     count_first=True)
                if kind == "scale":
                    if not all(np.isfinite(float(s)) for s in vals):
                        raise ValueError(f"{name} must be finite")
                    vals = torch.tensor([float(s) for s in vals], dtype=torch.float32)
                else:
                    vals = torch.tensor([int(s) for s in vals], dtype=torch.int64)
            key = (B, kind)
            if key not in self._rowbuf:
                self._rowbuf[key] = torch.empty(B, dtype=dtype, device=dev)
            self._rowbuf[key].copy_(vals)
            return self._rowbuf[key]

        s_rows = c_rows = None
        if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)):
            s_rows = rows("scale", scale, torch.float32, "scale")
        if clip_ids is not None:
            if clip_base:
                raise ValueError("clip_ids and a non-zero clip_base do not go together: the ids are global clip indices")
            c_rows = rows("clip_ids", clip_ids, torch.int64, "clip")
        if s_rows is None and c_rows is None:
            return None, float(scale), held
        rs = L.Rows(s_rows.data_ptr() if s_rows is not None else None, c_rows.data_ptr() if c_rows is not None else None)
        return rs, 0.0 if s_rows is not None else float(scale), held + [s_rows, c_rows]

    @staticmethod
    def _windows_struct(windows, B: int, T: int):
        """validate the window starts of a joint call - B rows = nw windows (row = w * Bc + b) of T tokens each - and lay them out as
        vb_windows (a host array, read during the call).  The rules are the library's (include/versband_hip.h), stated here first so that
        the error names the caller's argument.  Returns (struct, the array to hold)."""
        starts = [int(s) for s in _checked_list("windows", windows, "integers", None, "a sequence of window starts", " (the window starts)")]
        nw = len(starts)
        if not 1 <= nw <= 64:
            raise ValueError(f"windows: {nw} windows (1..64)")
        if B % nw:
            raise ValueError(f"windows: {B} rows are not {nw} windows of whole clips (B % nw != 0)")
        if starts[0] < 0:
            raise ValueError(f"windows: window 0 starts at {starts[0]}")
        for w in range(nw - 1):
            if starts[w + 1] <= starts[w]:
                raise ValueError(f"windows: window {w + 1} at {starts[w + 1]} does not come after window {w} at {starts[w]} (descending starts)")
            if starts[w + 1] > starts[w] + T:
                raise ValueError(f"windows: a gap between window {w} at {starts[w]} (length {T}) and window {w + 1} at {starts[w + 1]}")
            if w + 2 < nw and starts[w + 2] < starts[w] + T:
                raise ValueError(f"windows: window {w + 2} at {starts[w + 2]} reaches into window {w} at {starts[w]} (length {T}): "
                                 "a token under three windows")
        arr = (C.c_int32 * nw)(*starts)
        return L.Windows(arr, nw), arr

    _lens_struct = staticmethod(_lens_struct)       # (the name the call sites and the tests use)

    @staticmethod
    def _window_rows_struct(window_rows, B: int, T: int, lens=None, windows=None):
        """validate the per-row window plan of a joint call over clips of different lengths - window_rows = (group, start), B integers
        each: row r is a window of long clip group[r] over its tokens [start[r], start[r] + len[r]), len[r] = lens[r] (the call's row
        lengths) or T - and lay it out as vb_window_rows (two host arrays, read during the call).  The rules are the library's
        (include/versband_hip.h), stated here first so that the error names the caller's argument and the row.  Returns (struct, the
        arrays to hold, the consensus pairs [(ra, rb, off_a, ov)])."""
        try:
            group, start = window_rows
        except (TypeError, ValueError):
            raise TypeError("window_rows must be a pair (group, start) of per-row sequences") from None
        if group is None or start is None:
            raise ValueError("window_rows: group and start must both be given (row 0 has no plan)")
        if windows is not None and len(list(windows)) > 1:
            raise ValueError("window_rows and windows do not go together: one plan describes the rows, not two (row 0 would stand under both)")
        if B > 64:
            raise ValueError(f"window_rows: {B} rows (at most 64; row 64 has no slot in the table)")
        group = [int(v) for v in _checked_list("window_rows group", group, "integers", (B, "rows"), f"a sequence of {B} clip ids", " (one clip id per row)")]
        start = [int(v) for v in _checked_list("window_rows start", start, "integers", (B, "rows"), f"a sequence of {B} window starts",
                                               " (one window start per row)")]
        ln = list(lens) if lens is not None else [T] * B
        last, pairs = {}, []               # group -> (its last row, the row before that)
        for r in range(B):
            if start[r] < 0:
                raise ValueError(f"window_rows: start[{r}] = {start[r]} (row {r} starts before its clip)")
            ra, rz = last.get(group[r], (None, None))
            last[group[r]] = (r, ra)
            if ra is None:
                continue
            end_a = start[ra] + ln[ra]
            if start[r] <= start[ra]:
                raise ValueError(f"window_rows: row {r} at {start[r]} does not come after row {ra} at {start[ra]} of group {group[r]} "
                                 "(rows of a group ascend)")
            if start[r] > end_a:
                raise ValueError(f"window_rows: a gap between row {ra} at {start[ra]} (length {ln[ra]}) and row {r} at {start[r]} of group {group[r]}")
            ov = end_a - start[r]
            if ov > ln[r]:
                raise ValueError(f"window_rows: row {r} of length {ln[r]} lies inside its overlap of {ov} tokens with row {ra} (group {group[r]})")
            if rz is not None and start[r] < start[rz] + ln[rz]:
                raise ValueError(f"window_rows: row {r} at {start[r]} reaches into row {rz} at {start[rz]} (length {ln[rz]}) of group {group[r]}: "
                                 "a token under three rows")
            if ov > 0:
                pairs.append((ra, r, ln[ra] - ov, ov))
        ga, sa = (C.c_int32 * B)(*group), (C.c_int32 * B)(*start)
        return L.WindowRows(ga, sa), (ga, sa), pairs

    @staticmethod
    def _guidance_struct(guidance, n: int):
        """validate per-step guidance weights - n finite numbers in [0, 16], the library's rules (include/versband_hip.h), stated here
        first so that the error names the caller's argument - and lay them out as vb_guidance (a host array, read during the call).
        All ones is the plain call.  Returns (struct or None, the array to hold)."""
        vals = [float(np.float32(v)) for v in _checked_list("guidance", guidance, "numbers", (n, "steps"), f"a sequence of {n} step weights",
                                                            " (one weight per step)")]
        for k, v in enumerate(vals):
            if not (np.isfinite(v) and 0.0 <= v <= 16.0):
                raise ValueError(f"guidance[{k}] = {v} is not a finite value in [0, 16]")
        if all(v == 1.0 for v in vals):
            return None, None
        arr = (C.c_float * n)(*vals)
        return L.Guidance(arr), arr

    def sample_cfg(self, x0: Tensor, cond: dict, t_idx_table: Sequence[int], dt_table: Sequence[float], scale,
                   noise=None, seed: int = 0, clip_base: int = 0, return_traj: bool = False, keep=None, clip_ids=None, windows=None,
                   guidance=None, lengths=None, window_rows=None):
        """n Euler steps with classifier-free guidance; x0 [B,C,T] is not modified.
        scale: one number for the batch, or B values (sequence / float32 tensor): row b is guided by scale[b].  clip_ids: B global clip
        indices (sequence / int64 tensor): row b draws its router noise as clip clip_ids[b] instead of clip_base + b (vb_rows).
        keep = (ref [B,C,T], x0 [B,C,T], mask [B,T] in [0,1], t_next [n], sigma_min) or a dict of those names holds the masked tokens on
        the probability path t ref + (1 - (1 - sigma_min) t) x0 after every step (vb_keep; t_next = model.euler_times).
        windows: a sequence of nw ascending window starts - the B rows are then nw windows (row = w * (B // nw) + b, T tokens each) of
        B // nw long clips, and after every step the overlapping tokens of neighbouring windows take one consensus value, so they are
        bit-identical in the result and in every trajectory state (vb_windows).  Combines with all of the above; scale,
        clip_ids and keep stay per ROW.
        guidance: one weight in [0, 16] per step (vb_guidance) - step k runs under the effective scale 1 + guidance[k] * (scale - 1):
        1 is the plain step, 0 evaluates the conditional branch alone (about half the step's network time), anything between or
        beyond scales the guidance.  All ones or None is the plain call; with one branch (nb = 1) the weights are checked and unused.
        Combines with all of the above.
        lengths: B row lengths in latent tokens (vb_lens), the ones the conditioning was made with - clips of different lengths as rows of
        one call, padded to T: row b's first lengths[b] tokens are the call on that clip alone, the rest of x0's row is never read into
        them.  The padding of the returned latent (and trajectory) is zero-filled.  Combines with scale, clip_ids, keep and guidance
        (all per row or per step); not with more than one window.
        window_rows = (group, start), B integers each: joint windows of clips of DIFFERENT lengths (vb_window_rows) - row r is a window of
        long clip group[r] over its tokens [start[r], start[r] + lengths[r]) (T without lengths); rows of a group ascend in start and need
        not be adjacent.  Neighbouring rows of a group take one consensus value in their overlap after every step, exactly as with
        windows=; the rows of a group equal the call on that group's rows alone with the same clip_ids.  Combines with lengths, scale,
        clip_ids, keep and guidance; not with more than one window in windows=."""
        dev = self.ctx.device
        B, nb, T, Lc = cond["B"], cond["nb"], cond["T"], cond["L"]
        ls, held_lens, lens = DiTEngine._lens_struct(lengths, B, T, windows=windows, cond=cond)
        rstruct, held_wrows = (self._window_rows_struct(window_rows, B, T, lens, windows)[:2] if window_rows is not None else (None, None))
        wstruct, held_win = self._windows_struct(windows, B, T) if windows is not None else (None, None)
        rs, scale, held_rows = self._rows_struct(scale, clip_ids, B, clip_base)
        self._check_cond(cond)
        xkey = (B, self.cfg.in_channels, T)
        assert tuple(x0.shape) == xkey, (tuple(x0.shape), xkey)
        if xkey not in self._xbuf:
            self._xbuf[xkey] = torch.empty(xkey, dtype=torch.float32, device=dev)
        x = self._xbuf[xkey]            # the state the solver integrates in place; the caller gets a copy
        x.copy_(x0.to(dev, torch.float32))
        n = len(t_idx_table)
        tkey = (tuple(int(v) for v in t_idx_table), tuple(float(v) for v in dt_table))
        tt, dd = _device_tables(self._tables, tkey, lambda: (torch.tensor(tkey[0], dtype=torch.int64, device=dev),
                                                             torch.tensor(tkey[1], dtype=torch.float32, device=dev)))
        gs, held_guid = self._guidance_struct(guidance, n) if guidance is not None else (None, None)
        ks, held_keep = self._keep_struct(keep, B, T, n) if keep is not None else (None, None)
        ns, held = self._noise_struct(noise, seed, clip_base, 0)
        traj = torch.empty(n + 1, *x.shape, dtype=torch.float32, device=dev) if return_traj else None
        ws = self._workspace(B, nb, T, Lc)
        if rstruct is not None:         # the per-row window plan has its own entry point, vb_sample_cfg_lens's arguments plus the block
            L.check(self.ctx.lib.vb_sample_cfg_window_rows(self.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, nb, T, Lc, n, L.ptr(tt), L.ptr(dd),
                                                           float(scale), _ref(rstruct), _ref(ls), _ref(gs), _ref(wstruct), _ref(rs), _ref(ks),
                                                           _ref(ns), L.ptr(traj), L.ptr(ws), L.stream_ptr()), "vb_sample_cfg_window_rows")
        else:                           # every other call goes where it always went: an absent option is a null pointer, which is all the older entry points pass in its place
            L.check(self.ctx.lib.vb_sample_cfg_lens(self.ctx.handle, L.ptr(x), L.ptr(cond["buf"]), B, nb, T, Lc, n, L.ptr(tt), L.ptr(dd),
                                                    float(scale), _ref(ls), _ref(gs), _ref(wstruct), _ref(rs), _ref(ks), _ref(ns), L.ptr(traj),
                                                    L.ptr(ws), L.stream_ptr()), "vb_sample_cfg_lens")
        x = x.clone()
        if lens is not None:            # the padding tokens are unspecified (vb_lens): the caller gets a defined tensor
            for b, n_b in enumerate(lens):
                x[b, :, n_b:] = 0
                if traj is not None:
                    traj[:, b, :, n_b:] = 0
        return (x, traj) if return_traj else x

    def graphs(self) -> int:
        """instantiated hipGraphs of the sampler loop this engine's context holds (0 = every call ran eagerly)"""
        return int(self.ctx.lib.vb_sample_graphs(self.ctx.handle))


class T5Engine:
    """transformers.T5EncoderModel(input_ids).last_hidden_state on the HIP library: token ids [B,L] ->
    [B,L,d_model] fp32.  `sd` uses the HF state_dict keys; heads / eps / bucket parameters come from the HF config."""

    def __init__(self, ctx: Context, sd: Dict[str, Tensor], num_heads: int = 16, d_kv: int = 64, eps: float = 1e-6, max_len: int = 128,
                 num_buckets: int = 32, max_distance: int = 128):
        ctx = Context(ctx.device)
        self.ctx = ctx
        top, layers = pack.pack_t5(sd, ctx.device, num_heads, max_len, num_buckets, max_distance)
        self._keep = (top, layers)
        d_ff = sd["encoder.block.0.layer.1.DenseReluDense.wi_0.weight"].shape[0]
        self.cfg = L.T5Config(vocab=top["embed"].shape[0], d_model=top["embed"].shape[1], d_kv=d_kv, heads=num_heads, d_ff=d_ff,
                              layers=len(layers), eps=eps)
        w = L.T5Weights()
        w.embed, w.pos_bias, w.pos_len = top["embed"].data_ptr(), top["pos_bias"].data_ptr(), max_len
        w.final_ln, w.ones = top["final_ln"].data_ptr(), top["ones"].data_ptr()
        for i, lw in enumerate(layers):
            for f in L.T5_LAYER_FIELDS:
                setattr(w.layers[i], f, lw[f].data_ptr())
        L.check(ctx.lib.vb_t5_load(ctx.handle, C.byref(self.cfg), C.byref(w)), "vb_t5_load")
        self._ws = None

    def encode(self, ids: Tensor) -> Tensor:
        dev = self.ctx.device
        ids = ids.to(dev, torch.int64).contiguous()
        B, Lc = ids.shape
        n = self.ctx.lib.vb_t5_workspace_bytes(C.byref(self.cfg), B, Lc)
        if self._ws is None or self._ws.numel() < n:
            self._ws = torch.empty(n, dtype=torch.uint8, device=dev)
        out = torch.empty(B, Lc, self.cfg.d_model, dtype=torch.float32, device=dev)
        L.check(self.ctx.lib.vb_t5_encode(self.ctx.handle, L.ptr(ids), B, Lc, L.ptr(out), L.ptr(self._ws), L.stream_ptr()), "vb_t5_encode")
        return out


# ---------------------------------------------------------------------------
# conv nets
# ---------------------------------------------------------------------------


def mf_conv_eligible(w: Tensor, Ci: int, Co: int, k: int, dil: int, in_act: int, upsample2: int, out_transposed: int, tr_stride: int,
                     in_stride: int) -> bool:
    """Whether an "fp32mf" convolution also carries F(2,3) minimal-filtering weights: weights packed [k][Ci][Co], stride 1, no
    upsampling, channel-major output, k = 3 / 5 / 7 / 11 with dil <= 8 and (k - 1) * dil <= 60, Ci % 16 == 0, Co % 4 == 0, Co >= 64
    (conv1d_f32w_kernel runs 64- or 128-channel output tiles), input activation none / LeakyReLU.  launch_conv1d re-checks at run time
    what depends on T and on the buffers (T % 4 == 0, 16-byte aligned x / out / res / weights) and runs the direct kernels on w where
    those fail; it would also take Co >= 32."""
    return (tr_stride == 1 and in_stride == 1 and not upsample2 and not out_transposed and k in (3, 5, 7, 11) and dil <= 8 and
            (k - 1) * dil <= 60 and Ci % 16 == 0 and Co % 4 == 0 and Co >= 64 and in_act in (L.ACT_NONE, L.ACT_LRELU) and
            tuple(w.shape) == (k, Ci, Co))


class _Precision(NamedTuple):
    """one row of NET_PRECISIONS: everything NetBuilder and the builders decide by a precision's name"""
    x3_like: bool               # the op list's shape: fused input transforms, per-clip weights as split planes
    xt_like: bool               # wide layers read pre-activated transposed planes (VB_OP_XT_PLANES)
    wfmt: int                   # static weights: their format (a layer has to qualify for WFMT_MF, mf_conv_eligible, or stays WFMT_F32),
    pack: Optional[Callable]    # its packer, (w, device) -> (the tensor to keep, ci_pad or None) - None: plain fp32, w itself -
    slot: str                   # and the vb_net_op field the packed weights travel in, which respair copies to w2
    keeps_fp32: bool            # an op that asks for the fp32 copy beside its packed weights gets it (False: only an op that reads w,
                                # one output channel)
    buf_wfmt: int               # per-batch weights in a buffer: their format
    xt_planes: int              # planes xt_planes writes: split-bf16 hi / lo, or ONE RN-bf16 plane (WFMT_BF16, half the bytes)
    fp32_pairs: Optional[str]   # HiFi-GAN pair fusion: None = the window-staged rule (build_hifigan's fuse_pairs, reach <= 64); a string =
                                # the fp32 DMA rule, for the channel counts of VB_FP32_PAIRS, this string by default


def _pack_x3(w: Tensor, device):
    return pack.pack_conv_x3(w.to(device))


def _pack_bf16(w: Tensor, device):
    return pack.pack_conv_bf16(w.to(device))


def _pack_mf(w: Tensor, device):
    return pack.pack_conv_mf(w.permute(2, 1, 0)).to(device, torch.float32).contiguous(), None      # (w arrives packed [k][Ci][Co])


# The conv-net precisions; a new one is a new row.
# "split": bf16x3 MFMA conv kernels (fp32-class); "fp32": the exact-fp32 MFMA kernels; "fp32mf": the fp32 op list in which the
# layers of mf_conv_eligible and the 32 / 64-channel pairs run F(2,3) minimal filtering (fp32 products, ~1.45x fewer);
# "bf16": the split op list without the DMA-fed input planes, every static-weight convolution and 32 / 64-channel pair in ONE
# bf16 pass (RN-bf16 weights x RN-bf16 activated input, fp32 accumulation: outside the 1e-3 parity contract);
# "bf16xt": the same arithmetic on the split op list's SHAPE - every wide layer's input is activated, rounded and transposed once
# into ONE bf16 plane (VB_OP_XT_PLANES with WFMT_BF16) and the BF16 convolution reads it by DMA (a one-pass GEMM where it qualifies)
NET_PRECISIONS: Dict[str, _Precision] = {
    #                    x3_like xt_like wfmt       pack        slot   keeps_fp32 buf_wfmt    xt_planes fp32_pairs
    "split":  _Precision(True,  True,  L.WFMT_X3,   _pack_x3,   "w_x3", True,  L.WFMT_BUF_X3,  2, None),
    "fp32":   _Precision(False, False, L.WFMT_F32,  None,       "w",    True,  L.WFMT_BUF_F32, 2, "32,64"),
    "fp32mf": _Precision(False, False, L.WFMT_MF,   _pack_mf,   "w_mf", True,  L.WFMT_BUF_F32, 2, "32"),
    "bf16":   _Precision(True,  False, L.WFMT_BF16, _pack_bf16, "w_x3", False, L.WFMT_BUF_X3,  2, None),
    "bf16xt": _Precision(True,  True,  L.WFMT_BF16, _pack_bf16, "w_x3", False, L.WFMT_BUF_X3,  1, None),
}

# The A/B switches of the conv-net builders: environment variables that keep a measured-against op list, or a tuning knob, alive.
# Every read goes through _switch: the first four when a builder runs, VB_XT_MIN_CO when this module is imported.
_SWITCHES = {
    # exact-fp32 modes: the channel counts whose ResBlock1 pairs run fused (respair_f32_kernel), "32,64" / "" for A/B runs.
    # (fp32mf: the 32-channel pairs run respair_f32w_kernel - minimal filtering in both convolutions, intermediate in LDS; the 64-channel pairs run
    #  as two unfused minimal-filtering launches: faster than the direct fused pair (1201 -> 1232 mel-s/s) AND than respair_f32w_kernel's 64-channel
    #  form (VB_FP32_PAIRS=32,64: 1196-1198 against 1224; a 2 x 2 wave grid leaves 16 MFMAs per ring step).
    #  A/Bs: profiles/r06_mf_pairs_ab.txt, profiles/r06_mf_pair32.txt)
    "VB_FP32_PAIRS": "channel counts of the fused fp32 pairs (default: the precision's row, \"32,64\" / fp32mf \"32\")",
    "VB_MF_PAIRS_OFF": "=1, fp32mf: the 32 / 64-channel pairs run the direct fused pair kernel, not minimal filtering",
    "VB_LRELU_IN_WINDOW": "=1: an unfused pair's inner LeakyReLU stays in the second convolution's window pass (the op list before round 6)",
    "VB_FP32_NO_PREPASS": "=1, exact-fp32 modes: GroupNorm (+ swish) stays in the register-staged convolution, no gn_apply pre-pass (the old op list)",
    "VB_XT_MIN_CO": "output channels from which a layer is wide (tuning knob, default 384; 256 / 128 would pull the wide vocoder stages in)",
}


def _switch(name: str, default: str = "") -> str:
    assert name in _SWITCHES, name
    return os.environ.get(name, default)


class NetBuilder:
    """Flattens a conv network into the vb_net_op list executed by the C++ runtime."""

    XT_MIN_CO = int(_switch("VB_XT_MIN_CO", "384"))

    def __init__(self, device, precision: str = "split"):
        assert precision in NET_PRECISIONS
        self.device = device
        self.precision = precision
        self.row = NET_PRECISIONS[precision]
        self.ops: List[L.NetOp] = []
        self.bufs: List[Tuple[int, int, int]] = []
        self.free: Dict[Tuple[int, int, int], List[int]] = {}
        self.keep: List[Tensor] = []
        self._aa_filter: Optional[Tensor] = None        # (BigVGAN's anti-aliasing filter, made by the first aa_act)

    def buf(self, channels: int, tmul: int, square: bool = False) -> int:
        key = (channels, tmul, int(square))
        if self.free.get(key):
            return self.free[key].pop()
        self.bufs.append(key)
        return len(self.bufs) - 1

    def release(self, b: int):
        if b >= 0:
            self.free.setdefault(self.bufs[b], []).append(b)

    def _t(self, t: Optional[Tensor]):
        if t is None:
            return None
        t = t.to(self.device, torch.float32).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def gn_stats(self, x: int, channels: int, groups: int = 32) -> int:
        st = self.buf(2 * groups, 1)
        op = L.NetOp(kind=L.OP_GN_STATS, x=x, out=-1, res=-1, stats=st, w_buf=-1, Ci=channels, gn_groups=groups)
        self.ops.append(op)
        return st

    def split_planes(self, x: int, out: int, rows: int, cols: int):
        """f32 [B][rows][cols] buffer -> split-bf16 planes [2][B][rows][roundup(cols,32)] (-1 = the buffer's time length)."""
        self.ops.append(L.NetOp(kind=L.OP_SPLIT_PLANES, x=x, out=out, res=-1, stats=-1, w_buf=-1, Ci=cols, Co=rows))

    def weights(self, w: Optional[Tensor], w_buf: int = -1, mf: bool = False, fallback: bool = True) -> dict:
        """One layer's weights packed for this builder's precision -> the op's format fields (include/versband_hip.h, VB_WFMT_*).
        w: fp32 packed [phase][tap][Ci][Co]; w_buf: per-batch weights in a buffer instead (split: written by split_planes); mf: the
        layer qualifies for minimal filtering (fp32mf only); fallback: an X3 / MF conv keeps w as well (what the one-output-channel
        kernel and the direct kernels read)."""
        row = self.row
        if w_buf != -1:
            return dict(wfmt=row.buf_wfmt)
        if row.pack is None or (row.wfmt == L.WFMT_MF and not mf):
            return dict(wfmt=L.WFMT_F32, w=self._t(w))
        packed, ci_pad = row.pack(w, self.device)
        self.keep.append(packed)
        f = {"wfmt": row.wfmt, row.slot: packed.data_ptr()}
        if ci_pad is not None:
            f["ci_pad"] = ci_pad
        if fallback and (row.keeps_fp32 or w.shape[-1] == 1):
            f["w"] = self._t(w)
        return f

    def respair(self, x: int, out: int, ch: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, k: int, dil: int, slope: float,
                alpha: float, beta: float):
        """Fused HiFi-GAN ResBlock1 pair (w1/w2 fp32 packed [k][Ci][Co]); narrow stages only (ch = 32 or 64; fp32 mode: 32 / 64 / 128).
        fp32mf: the 32 / 64-channel pairs of k = 3 / 7 / 11 run minimal filtering in both convolutions (respair_f32w.hip),
        VB_MF_PAIRS_OFF=1 the direct pair kernel."""
        mf = ch in (32, 64) and k in (3, 7, 11) and not _switch("VB_MF_PAIRS_OFF")
        f = self.weights(w1, mf=mf, fallback=False)
        slot = "w" if f["wfmt"] == L.WFMT_F32 else self.row.slot        # the second convolution's weights go from there to w2
        f["w2"] = self.weights(w2, mf=mf, fallback=False)[slot]
        self.ops.append(L.NetOp(kind=L.OP_RESPAIR, x=x, out=out, res=-1, stats=-1, w_buf=-1, bias=self._t(b1), bias2=self._t(b2), Ci=ch, Co=ch,
                                ksize=k, dil=dil, in_slope=slope, alpha=alpha, beta=beta, **f))

    def aa_act(self, x: int, out: int, ch: int, alpha: Tensor, beta: Optional[Tensor], logscale: bool):
        """BigVGAN Activation1d(Snake / SnakeBeta): out = down2(act(up2(x))) (alias_free_torch/act.py)."""
        if self._aa_filter is None:
            self._aa_filter = pack.kaiser_sinc_filter1d(0.25, 0.3, 12)
        a = alpha.float()
        b = a if beta is None else beta.float()
        if logscale:
            a, b = torch.exp(a), torch.exp(b)
        self.ops.append(L.NetOp(kind=L.OP_AA_ACT, x=x, out=out, res=-1, stats=-1, w_buf=-1, Ci=ch, gn_gamma=self._t(a),
                                gn_beta=self._t(1.0 / (b + 1e-9)), w=self._t(self._aa_filter)))

    def softmax_t(self, x: int, out: int):
        self.ops.append(L.NetOp(kind=L.OP_SOFTMAX_T, x=x, out=out, res=-1, stats=-1, w_buf=-1))

    def conv(self, x: int, out: int, Ci: int, Co: int, w: Optional[Tensor] = None, bias: Optional[Tensor] = None, k: int = 1,
             dil: int = 1, pad: int = 0, res: int = -1, stats: int = -1, gamma=None, beta_gn=None, in_act=L.ACT_NONE,
             in_slope=0.0, out_act=L.ACT_NONE, out_slope=0.0, upsample2=0, out_transposed=0, w_buf=-1, alpha=1.0, beta=0.0,
             acc_scale=1.0, tr_stride=1, tr_pad=0, tr_k=0, groups=32, in_stride=1, in_phase=0, x_is_planes=False):
        tmp = -1
        x_planes = int(bool(x_is_planes))
        if (self.row.xt_like and not x_planes and w is not None and w_buf == -1 and x >= 0 and Co >= self.XT_MIN_CO and Ci % 32 == 0
                and tr_stride == 1 and in_stride == 1 and pad <= 64 and (k - 1) * dil <= 64 and (k > 1 or in_act != L.ACT_NONE)):
            # wide layer (>= 3 output-channel tiles): the input is activated, split (bf16xt: rounded) and transposed ONCE (VB_OP_XT_PLANES)
            # and every tile of the convolution DMAs its window from there, instead of each tile redoing norm / swish / split while staging
            tmp = self.xt_planes(x, Ci, stats, gamma, beta_gn, in_act, in_slope, upsample2, groups)
            x, stats, gamma, beta_gn, in_act, x_planes = tmp, -1, None, None, L.ACT_NONE, 1
        if (not self.row.x3_like and in_act in (L.ACT_GN_SWISH, L.ACT_GN) and stats >= 0 and w is not None and w_buf == -1 and x >= 0
                and Ci % 16 == 0 and Co % 4 == 0 and in_stride == 1 and tr_stride == 1 and not _switch("VB_FP32_NO_PREPASS")):
            # exact-fp32 mode: GroupNorm (+ swish) is applied ONCE by gn_apply_kernel and the DMA-fed fp32 kernel (conv1d_f32g_kernel)
            # reads the activated tensor; the register-staged kernel redid norm + swish + expf for every output-channel tile
            # (12 times on the 1536-channel layers: 2.3 ms for an 85-GFLOP layer).
            tmp = self.gn_apply(x, Ci, stats, gamma, beta_gn, in_act, groups)
            x, stats, gamma, beta_gn, in_act = tmp, -1, None, None, L.ACT_NONE
        mf = w is not None and mf_conv_eligible(w, Ci, Co, k, dil, in_act, upsample2, out_transposed, tr_stride, in_stride)
        op = L.NetOp(kind=L.OP_CONV, x=x, out=out, res=res, stats=stats, w_buf=w_buf, bias=self._t(bias), gn_gamma=self._t(gamma),
                     gn_beta=self._t(beta_gn), Ci=Ci, Co=Co, ksize=k, dil=dil, pad=pad, upsample2=upsample2, in_act=in_act,
                     out_act=out_act, out_transposed=out_transposed, tr_stride=tr_stride, tr_pad=tr_pad, tr_k=tr_k, gn_groups=groups,
                     in_slope=in_slope, out_slope=out_slope, alpha=alpha, beta=beta, acc_scale=acc_scale, in_stride=in_stride,
                     in_phase=in_phase, x_planes=x_planes, **self.weights(w, w_buf, mf))
        self.ops.append(op)
        self.release(tmp)

    def xt_planes(self, x: int, channels: int, stats: int, gamma, beta_gn, act: int, slope: float, upsample2: int, groups: int = 32) -> int:
        """x -> new buffer of pre-activated, split-bf16, transposed planes with zero halo rows (VB_OP_XT_PLANES); bf16xt: the one-plane
        form (WFMT_BF16, a buffer of square = 4: half the bytes)."""
        one = self.row.xt_planes == 1
        out = self.buf(channels, self.bufs[x][1] * (2 if upsample2 else 1), 4 if one else 3)
        self.ops.append(L.NetOp(kind=L.OP_XT_PLANES, wfmt=L.WFMT_BF16 if one else L.WFMT_NONE, x=x, out=out, res=-1, stats=stats, w_buf=-1,
                                gn_gamma=self._t(gamma),
                                gn_beta=self._t(beta_gn), Ci=channels, gn_groups=groups, in_act=act, in_slope=slope, upsample2=upsample2))
        return out

    def gn_apply(self, x: int, channels: int, stats: int, gamma, beta_gn, act: int, groups: int = 32) -> int:
        """x -> new buffer holding GroupNorm(x) (act = ACT_GN) or swish(GroupNorm(x)) (ACT_GN_SWISH)."""
        out = self.buf(channels, self.bufs[x][1])
        self.ops.append(L.NetOp(kind=L.OP_GN_APPLY, x=x, out=out, res=-1, stats=stats, w_buf=-1, gn_gamma=self._t(gamma),
                                gn_beta=self._t(beta_gn), Ci=channels, gn_groups=groups, in_act=act))
        return out


class ConvNet:
    def __init__(self, ctx: Context, which: int, nb: NetBuilder, in_ch: int, out_ch: int, out_tmul: int, in_tmul: int = 1):
        ctx = Context(ctx.device)        # one program per (vb_ctx, slot): every net owns its handle
        self.ctx, self.which, self.nb = ctx, which, nb
        self.in_ch, self.out_ch, self.out_tmul, self.in_tmul = in_ch, out_ch, out_tmul, in_tmul
        ops = (L.NetOp * len(nb.ops))(*nb.ops)
        bufs = (L.BufDesc * max(1, len(nb.bufs)))(*[L.BufDesc(*b) for b in nb.bufs])
        L.check(ctx.lib.vb_net_load(ctx.handle, which, ops, len(nb.ops), bufs, len(nb.bufs), in_ch, out_ch, in_tmul, out_tmul),
                "vb_net_load")
        # scratch that is sized for a call's shape and made again when that changes: slot -> (the shape, the buffers).  Slots: "net" (the
        # plain workspace), "chunk" (the chunk scratch) and one per lengths entry point, under its own name
        self._scratch = {}

    def _cached(self, slot: str, key: Tuple[int, ...], make):
        if self._scratch.get(slot, (None, None))[0] != key:
            self._scratch[slot] = (key, make())
        return self._scratch[slot][1]

    def _bytes(self, n: int) -> Tensor:
        return torch.empty(max(n, 256), dtype=torch.uint8, device=self.ctx.device)

    def _workspace(self, B, T):
        return self._cached("net", (B, T), lambda: self._bytes(self.ctx.lib.vb_net_workspace_bytes(self.ctx.handle, self.which, B, T)))

    NET_NAMES = {L.NET_VAE: "VAE decoder", L.NET_VOCODER: "vocoder", L.NET_VAE_ENCODER: "VAE encoder"}

    def run(self, x: Tensor, lengths=None) -> Tensor:
        """lengths (vocoder only; vb_hifigan_forward_lens): one length in input frames per row - mels of different lengths padded to
        x.shape[-1] share the call.  Row b's first lengths[b] * out_tmul samples are the call on that clip alone (bit for bit when
        lengths[b] and x.shape[-1] agree mod 4, to fp32 roundoff otherwise: harness.plan_vocoder_calls groups rows accordingly), the rest
        of the row is zero, and the padding of x is never read.  None, or every row full, is the plain call."""
        x = x.to(self.ctx.device, torch.float32).contiguous()
        B, Cin, Tin = x.shape
        assert Cin == self.in_ch, (Cin, self.in_ch)
        if Tin % self.in_tmul:
            raise ValueError(f"input length {Tin} is not a multiple of {self.in_tmul}")
        T = Tin // self.in_tmul
        if lengths is not None:
            if self.which != L.NET_VOCODER:
                hint = "; the VAE decoder takes them through decode_lens" if self.which == L.NET_VAE else "; the VAE encoder takes them through encode_lens"
                raise ValueError(f"lengths: the {self.NET_NAMES[self.which]} takes equal-length rows only through run (row lengths reach the "
                                 f"vocoder net alone{hint})")
            lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (input frames per row)")
            if lens is not None:
                return self._lens_call("vb_hifigan_forward_lens", x, B, T, lens, hold)
        out = torch.empty(B, self.out_ch, T * self.out_tmul, dtype=torch.float32, device=self.ctx.device)
        ws = self._workspace(B, T)
        fn = {L.NET_VAE: self.ctx.lib.vb_vae_decode, L.NET_VOCODER: self.ctx.lib.vb_hifigan_forward,
              L.NET_VAE_ENCODER: self.ctx.lib.vb_vae_encode}[self.which]
        L.check(fn(self.ctx.handle, L.ptr(x), B, T, L.ptr(out), L.ptr(ws), L.stream_ptr()), "conv net run")
        return out

    def _chunk_scratch(self, B: int, tc: int):
        """(cin, cout) of the chunked entry points: one chunk with its halos, tc frames, of every row - gathered input, generator output"""
        dev = self.ctx.device
        return self._cached("chunk", (B, tc), lambda: (torch.empty(B * self.in_ch * tc, dtype=torch.float32, device=dev),
                                                       torch.empty(B * self.out_ch * tc * self.out_tmul, dtype=torch.float32, device=dev)))

    # the lengths entry points and the function that sizes each one's workspace (with B, T and, chunked, chunk and halo)
    LENS_WORKSPACE = {"vb_hifigan_forward_lens": "vb_hifigan_lens_workspace_bytes",
                      "vb_vae_decode_lens": "vb_vae_decode_lens_workspace_bytes",
                      "vb_vae_encode_lens": "vb_vae_encode_lens_workspace_bytes",
                      "vb_bigvgan_forward_lens": "vb_bigvgan_lens_workspace_bytes",
                      "vb_hifigan_forward_chunked_lens": "vb_hifigan_chunked_lens_workspace_bytes",
                      "vb_bigvgan_forward_chunked_lens": "vb_bigvgan_chunked_lens_workspace_bytes"}

    def _lens_call(self, name: str, x: Tensor, B: int, T: int, lens, hold, chunked: Tuple[int, ...] = ()) -> Tensor:
        """the lengths entry point `name` on rows x [B, in_ch, T * in_tmul] (contiguous fp32 on the device); lens / hold: the vb_lens struct and
        its host array (_lens_struct); chunked: (chunk, halo) for the chunked entry points, which also take the chunk scratch"""
        lib, handle = self.ctx.lib, self.ctx.handle
        out = torch.empty(B, self.out_ch, T * self.out_tmul, dtype=torch.float32, device=self.ctx.device)
        shape = (B, T) + tuple(chunked)
        ws = self._cached(name, shape, lambda: self._bytes(getattr(lib, self.LENS_WORKSPACE[name])(handle, *shape)))
        scratch = [L.ptr(t) for t in self._chunk_scratch(B, chunked[0] + 2 * chunked[1])] if chunked else []
        L.check(getattr(lib, name)(handle, L.ptr(x), *shape, C.byref(lens), L.ptr(out), L.ptr(ws), *scratch, L.stream_ptr()), name)
        del hold                         # (the host array of the lengths: read during the call only)
        return out

    def decode_lens(self, z: Tensor, lengths) -> Tensor:
        """VAE decoder only (vb_vae_decode_lens): z [B, zc, T] with one latent length per row - latents of different lengths padded to T
        share the call.  Row b's first 2 * lengths[b] mel frames are the decode of that clip alone (bit for bit when lengths[b] and T
        agree mod 4, to fp32 roundoff otherwise: harness.plan_decode_calls groups rows accordingly), the rest of the row is zero, and
        neither the padding of z nor anything in the workspace is read.  None, or every row full, is run(z)."""
        if self.which != L.NET_VAE:
            raise ValueError(f"decode_lens: the {self.NET_NAMES[self.which]} has no decode_lens (the VAE decoder alone; the vocoder takes "
                             f"row lengths through run(lengths=), the VAE encoder through encode_lens)")
        z = z.to(self.ctx.device, torch.float32).contiguous()
        B, Cin, T = z.shape
        assert Cin == self.in_ch, (Cin, self.in_ch)
        lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (latent tokens per row)")
        if lens is None:
            return self.run(z)
        return self._lens_call("vb_vae_decode_lens", z, B, T, lens, hold)

    def encode_lens(self, mel: Tensor, lengths) -> Tensor:
        """VAE encoder only (vb_vae_encode_lens): mel [B, in_ch, T * in_tmul] with one LATENT length per row - the unit of the sampler and
        of decode_lens - so mels of different lengths padded to T * in_tmul frames share the call and row b owns its first
        lengths[b] * in_tmul frames.  Row b's first lengths[b] columns of the moments [B, 2 * embed, T] are the encode of that clip alone
        (bit for bit when lengths[b] and T agree mod 4, to the precision's roundoff otherwise: harness.plan_encode_calls groups rows
        accordingly), the rest of the row is zero, and neither the padding of mel nor anything in the workspace is read.  None, or every
        row full, is run(mel)."""
        if self.which != L.NET_VAE_ENCODER:
            raise ValueError(f"encode_lens: the {self.NET_NAMES[self.which]} has no encode_lens (the VAE encoder alone; the vocoder takes "
                             f"row lengths through run(lengths=), the VAE decoder through decode_lens)")
        mel = mel.to(self.ctx.device, torch.float32).contiguous()
        B, Cin, Tin = mel.shape
        assert Cin == self.in_ch, (Cin, self.in_ch)
        if Tin % self.in_tmul:
            raise ValueError(f"encode_lens: input length {Tin} is not a multiple of {self.in_tmul} (mel frames per latent token)")
        T = Tin // self.in_tmul
        lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (latent tokens per row)")
        if lens is None:
            return self.run(mel)
        return self._lens_call("vb_vae_encode_lens", mel, B, T, lens, hold)

    def run_chunked(self, x: Tensor, chunk: int, halo: int, lengths=None) -> Tensor:
        """vocoder only: mel [B,80,T] -> wav [B,1,T*hop] in chunks of `chunk` frames with `halo` frames of context on both sides, the loop,
        the slicing and the stitching inside the library (vb_hifigan_forward_chunked); identical to run() when halo >= the receptive field.
        lengths (vb_hifigan_forward_chunked_lens): one length in mel frames per row - long mels of different lengths padded to T share
        the call.  Row b's first lengths[b] * out_tmul samples are the chunk loop over that clip alone on the same grid
        (harness.plan_chunk_calls; bit for bit in every chunk where the row's frames and the chunk's width agree mod 4 - always when chunk,
        halo, T and the lengths are multiples of 4 - to fp32 roundoff elsewhere), the rest of the row is zero, a row that ended before a
        chunk is not run in it, and the padding of x is never read.  None, or every row full, is the call without lengths."""
        assert self.which == L.NET_VOCODER
        x = x.to(self.ctx.device, torch.float32).contiguous()
        B, Cin, T = x.shape
        assert Cin == self.in_ch
        lens = hold = None
        if lengths is not None:
            if chunk < 1 or halo < 0:
                raise ValueError(f"run_chunked: chunk = {chunk}, halo = {halo} (chunk >= 1, halo >= 0)")
            lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (input frames per row)")
        if T <= chunk + 2 * halo:
            return self.run(x) if lens is None else self._lens_call("vb_hifigan_forward_lens", x, B, T, lens, hold)
        if lens is not None:
            return self._lens_call("vb_hifigan_forward_chunked_lens", x, B, T, lens, hold, (chunk, halo))
        tc = chunk + 2 * halo
        out = torch.empty(B, self.out_ch, T * self.out_tmul, dtype=torch.float32, device=self.ctx.device)
        cin, cout = self._chunk_scratch(B, tc)
        ws = self._workspace(B, tc)
        L.check(self.ctx.lib.vb_hifigan_forward_chunked(self.ctx.handle, L.ptr(x), B, T, chunk, halo, L.ptr(out), L.ptr(ws), L.ptr(cin), L.ptr(cout),
                                                        L.stream_ptr()), "vb_hifigan_forward_chunked")
        return out

    def vocode_lens(self, x: Tensor, lengths, chunk: Optional[int] = None, halo: int = 32) -> Tensor:
        """vocoder nets only (vb_bigvgan_forward_lens / vb_bigvgan_forward_chunked_lens): mel [B,80,T] with one length in mel frames per row
        -> wav [B,1,T*hop], for a program with BigVGAN's anti-aliased activations (VB_OP_AA_ACT, which run(lengths=) and
        run_chunked(lengths=) refuse; a HiFi-GAN program runs here as it does there).  Row b's first lengths[b] * out_tmul samples are
        the call on that clip alone - run(), or with chunk the loop of run_chunked() on the same grid (harness.plan_chunk_calls) - bit for
        bit when lengths[b] and T agree mod 4 (chunked: in every chunk where the row's frames and the chunk's width do; always when chunk,
        halo, T and the lengths are multiples of 4), to the precision's roundoff otherwise: harness.plan_vocoder_calls groups rows
        accordingly.  The rest of the row is zero and the padding of x is never read.  lengths None, or every row full, is run() /
        run_chunked()."""
        if self.which != L.NET_VOCODER:
            raise ValueError(f"vocode_lens: the {self.NET_NAMES[self.which]} has no vocode_lens (vocoder nets alone; the VAE decoder takes row "
                             f"lengths through decode_lens, the VAE encoder through encode_lens)")
        x = x.to(self.ctx.device, torch.float32).contiguous()
        B, Cin, T = x.shape
        assert Cin == self.in_ch, (Cin, self.in_ch)
        if chunk is not None and (chunk < 1 or halo < 0):
            raise ValueError(f"vocode_lens: chunk = {chunk}, halo = {halo} (chunk >= 1, halo >= 0)")
        lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (input frames per row)")
        if lens is None:
            return self.run(x) if chunk is None else self.run_chunked(x, chunk, halo)
        if chunk is None or T <= chunk + 2 * halo:
            return self._lens_call("vb_bigvgan_forward_lens", x, B, T, lens, hold)
        return self._lens_call("vb_bigvgan_forward_chunked_lens", x, B, T, lens, hold, (chunk, halo))


def _vae_block_builders(nb: "NetBuilder", g: Dict[str, Tensor]):
    """(cw, resblock, attnblock) emitting ResnetBlock1D (autoencoder1d.py:172-231) / AttnBlock1D (:233-274) ops into nb."""

    def cw(name):
        return pack.pack_conv(g[name + ".weight"]), g[name + ".bias"]

    def resblock(x, cin, tm, p):
        cout = g[p + "conv1.weight"].shape[0]
        st1 = nb.gn_stats(x, cin)
        t1 = nb.buf(cout, tm)
        w, b = cw(p + "conv1")
        kk = g[p + "conv1.weight"].shape[2]      # 3 in the decoder, ddconfig.kernel_size in the encoder (autoencoder1d.py:346-351)
        nb.conv(x, t1, cin, cout, w, b, k=kk, pad=kk // 2, stats=st1, gamma=g[p + "norm1.weight"], beta_gn=g[p + "norm1.bias"],
                in_act=L.ACT_GN_SWISH)
        nb.release(st1)
        st2 = nb.gn_stats(t1, cout)
        sc = x
        if (p + "nin_shortcut.weight") in g:
            sc = nb.buf(cout, tm)
            w, b = cw(p + "nin_shortcut")
            nb.conv(x, sc, cin, cout, w, b)
        out = nb.buf(cout, tm)
        w, b = cw(p + "conv2")
        kk = g[p + "conv2.weight"].shape[2]
        nb.conv(t1, out, cout, cout, w, b, k=kk, pad=kk // 2, res=sc, stats=st2, gamma=g[p + "norm2.weight"], beta_gn=g[p + "norm2.bias"],
                in_act=L.ACT_GN_SWISH)
        nb.release(st2); nb.release(t1)
        if sc != x:
            nb.release(sc)
        nb.release(x)
        return out, cout

    def attnblock(x, c, tm, p):
        # single-head attention over time (AttnBlock1D, autoencoder1d.py): both matrix products run as k=1 convs whose
        # "weights" are per-batch activations.  split mode: those activations are split into bf16 hi/lo planes on the
        # device (q as [T][C], v as [C][T padded to 32]) so the bf16x3 MFMA kernel does the products too.
        st = nb.gn_stats(x, c)
        split = nb.row.x3_like      # (bf16: the per-clip products stay on the bf16x3 kernel, the q / k / v projections fuse the norm)
        q, k, v = nb.buf(c, tm), nb.buf(c, tm), nb.buf(c, tm)
        gam, bet = g[p + "norm.weight"], g[p + "norm.bias"]
        xn = nb.xt_planes(x, c, st, gam, bet, L.ACT_GN, 0.0, 0) if (nb.row.xt_like and c >= nb.XT_MIN_CO and c % 32 == 0) else -1
        for name, dst, tr in (("q", q, 1 if split else 0), ("k", k, 0), ("v", v, 0 if split else 1)):
            w, b = cw(p + name)
            if xn >= 0:
                nb.conv(xn, dst, c, c, w, b, out_transposed=tr, x_is_planes=True)
            else:
                nb.conv(x, dst, c, c, w, b, stats=st, gamma=gam, beta_gn=bet, in_act=L.ACT_GN, out_transposed=tr)
        nb.release(xn)
        s = nb.buf(0, tm, True)
        tmp = []
        if split:
            qp, vp = nb.buf(c, tm), nb.buf(c, tm, 2)
            nb.split_planes(q, qp, rows=-1, cols=c)                            # q^T [T][C] -> planes
            nb.split_planes(v, vp, rows=c, cols=-1)                            # v [C][T] -> planes, T padded
            tmp = [qp, vp]
            nb.conv(k, s, c, -1, w_buf=qp, acc_scale=float(int(c) ** (-0.5)))
        else:
            nb.conv(k, s, c, -1, w_buf=q, acc_scale=float(int(c) ** (-0.5)))  # w[b,i,j] = sum_c q[c,i] k[c,j] * C^-0.5
        pT = nb.buf(0, tm, True)
        nb.softmax_t(s, pT)
        a = nb.buf(c, tm)
        if split:
            nb.conv(pT, a, -1, c, w_buf=vp)
        else:
            nb.conv(pT, a, -1, c, w_buf=v)                                     # h[c,i] = sum_j v^T[j,c] P[i,j]
        out = nb.buf(c, tm)
        w, b = cw(p + "proj_out")
        nb.conv(a, out, c, c, w, b, res=x)
        for t in [st, q, k, v, s, pT, a, x] + tmp:
            nb.release(t)
        return out

    return cw, resblock, attnblock


def build_vae_decoder(ctx: Context, sd: Dict[str, Tensor], scale_factor: float = 1.0, precision: str = "split") -> ConvNet:
    """AutoencoderKL.decode (autoencoder1d.py:55-58) + Decoder1D.forward (:480-512) as an op list.
    The structure (levels, shortcut convs, attention blocks, which level upsamples) is read off the
    key names, exactly what load_state_dict would accept."""
    nb = NetBuilder(ctx.device, precision)
    g = sd
    cw, resblock, attnblock = _vae_block_builders(nb, g)

    zc = g["post_quant_conv.weight"].shape[1]
    h = nb.buf(g["post_quant_conv.weight"].shape[0], 1)
    w, b = cw("post_quant_conv")
    nb.conv(L.BUF_INPUT, h, zc, g["post_quant_conv.weight"].shape[0], w, b, acc_scale=1.0 / float(scale_factor))
    w, b = cw("decoder.conv_in")
    c = g["decoder.conv_in.weight"].shape[0]
    kk = g["decoder.conv_in.weight"].shape[2]
    h2 = nb.buf(c, 1)
    nb.conv(h, h2, g["decoder.conv_in.weight"].shape[1], c, w, b, k=kk, pad=kk // 2)
    nb.release(h)
    h, tm = h2, 1
    h, c = resblock(h, c, tm, "decoder.mid.block_1.")
    h = attnblock(h, c, tm, "decoder.mid.attn_1.")
    h, c = resblock(h, c, tm, "decoder.mid.block_2.")
    levels = sorted({int(k.split(".")[2]) for k in g if k.startswith("decoder.up.")})
    for lvl in reversed(levels):
        nblk = len({int(k.split(".")[4]) for k in g if k.startswith(f"decoder.up.{lvl}.block.")})
        for bi in range(nblk):
            h, c = resblock(h, c, tm, f"decoder.up.{lvl}.block.{bi}.")
            if f"decoder.up.{lvl}.attn.{bi}.norm.weight" in g:
                h = attnblock(h, c, tm, f"decoder.up.{lvl}.attn.{bi}.")
        if f"decoder.up.{lvl}.upsample.conv.weight" in g:
            w, b = cw(f"decoder.up.{lvl}.upsample.conv")
            h2 = nb.buf(c, tm * 2)
            nb.conv(h, h2, c, c, w, b, k=3, pad=1, upsample2=1)
            nb.release(h)
            h, tm = h2, tm * 2
    st = nb.gn_stats(h, c)
    w, b = cw("decoder.conv_out")
    co, kk = g["decoder.conv_out.weight"].shape[0], g["decoder.conv_out.weight"].shape[2]
    nb.conv(h, L.BUF_OUTPUT, c, co, w, b, k=kk, pad=kk // 2, stats=st, gamma=g["decoder.norm_out.weight"],
            beta_gn=g["decoder.norm_out.bias"], in_act=L.ACT_GN_SWISH)
    return ConvNet(ctx, L.NET_VAE, nb, zc, co, tm)


def build_vae_encoder(ctx: Context, sd: Dict[str, Tensor], precision: str = "split") -> ConvNet:
    """AutoencoderKL.encode up to the moments (autoencoder1d.py:49-53: Encoder1D.forward :383-409, then quant_conv :30):
    mel [B,in_ch,T_mel] -> [B, 2*embed_dim, T_mel / 2^len(down_layers)].  Structure read off the key names.
    Downsample1D (:294-313: pad right by one, Conv1d k3 stride 2) runs as two polyphase convolutions on the same kernels:
    out[n] = w0 x[2n] + w2 x[2n+2]  (taps 0 and 2 over the even samples)  +  w1 x[2n+1]  (tap 1 over the odd samples)."""
    nb = NetBuilder(ctx.device, precision)
    g = sd
    cw, resblock, attnblock = _vae_block_builders(nb, g)
    levels = sorted({int(k.split(".")[2]) for k in g if k.startswith("encoder.down.")})
    n_down = sum(1 for lvl in levels if f"encoder.down.{lvl}.downsample.conv.weight" in g)
    tm = 2 ** n_down
    w, b = cw("encoder.conv_in")
    cin, c, kk = g["encoder.conv_in.weight"].shape[1], g["encoder.conv_in.weight"].shape[0], g["encoder.conv_in.weight"].shape[2]
    h = nb.buf(c, tm)
    nb.conv(L.BUF_INPUT, h, cin, c, w, b, k=kk, pad=kk // 2)
    for lvl in levels:
        nblk = len({int(k.split(".")[4]) for k in g if k.startswith(f"encoder.down.{lvl}.block.")})
        for bi in range(nblk):
            h, c = resblock(h, c, tm, f"encoder.down.{lvl}.block.{bi}.")
            if f"encoder.down.{lvl}.attn.{bi}.norm.weight" in g:
                h = attnblock(h, c, tm, f"encoder.down.{lvl}.attn.{bi}.")
        if f"encoder.down.{lvl}.downsample.conv.weight" in g:
            wd, bd = g[f"encoder.down.{lvl}.downsample.conv.weight"].float(), g[f"encoder.down.{lvl}.downsample.conv.bias"]
            assert wd.shape[2] == 3 and tm % 2 == 0
            h2 = nb.buf(c, tm // 2)
            nb.conv(h, h2, c, c, pack.pack_conv(wd[:, :, 0::2].contiguous()), bd, k=2, pad=0, in_stride=2, in_phase=0)
            nb.conv(h, h2, c, c, pack.pack_conv(wd[:, :, 1:2].contiguous()), None, k=1, pad=0, in_stride=2, in_phase=1, beta=1.0)
            nb.release(h)
            h, tm = h2, tm // 2
    h, c = resblock(h, c, tm, "encoder.mid.block_1.")
    h = attnblock(h, c, tm, "encoder.mid.attn_1.")
    h, c = resblock(h, c, tm, "encoder.mid.block_2.")
    st = nb.gn_stats(h, c)
    w, b = cw("encoder.conv_out")
    co, kk = g["encoder.conv_out.weight"].shape[0], g["encoder.conv_out.weight"].shape[2]
    m = nb.buf(co, tm)
    nb.conv(h, m, c, co, w, b, k=kk, pad=kk // 2, stats=st, gamma=g["encoder.norm_out.weight"], beta_gn=g["encoder.norm_out.bias"],
            in_act=L.ACT_GN_SWISH)
    w, b = cw("quant_conv")
    nb.conv(m, L.BUF_OUTPUT, co, g["quant_conv.weight"].shape[0], w, b)
    assert tm == 1
    return ConvNet(ctx, L.NET_VAE_ENCODER, nb, cin, g["quant_conv.weight"].shape[0], 1, in_tmul=2 ** n_down)


def _wt(sd: Dict[str, Tensor], name: str) -> Tensor:
    """a vocoder layer's weight: stored plain, or as a weight-norm pair that is folded here"""
    if name + ".weight" in sd:
        return sd[name + ".weight"].float()
    return pack.fold_weight_norm(sd[name + ".weight_g"].float(), sd[name + ".weight_v"].float())


def _wb(sd: Dict[str, Tensor], name: str) -> Tuple[Tensor, Tensor]:
    """a vocoder convolution's (packed weight, bias), the two arguments of NetBuilder.conv / respair"""
    return pack.pack_conv(_wt(sd, name)), sd[name + ".bias"]


def _vocoder_walk(ctx: Context, nb: NetBuilder, sd: Dict[str, Tensor], hp: dict, ups: str, ups_act: dict, step, post) -> ConvNet:
    """The walk HiFi-GAN and BigVGAN share: conv_pre; per stage i a transposed conv (key ups.format(i), input activation ups_act) and
    the nk residual blocks of the stage averaged into one buffer; conv_post + tanh.  step(p, m, r, dst, ch, tm, rk, d, al, be) emits step m
    (kernel rk, dilation d) of the block with key prefix p, reading r and leaving al * (r + ...) + be * dst in dst; post(x, ch, tm) gives
    conv_post's input buffer and its input-activation arguments.  The order of nb.buf, nb.release and the ops is the order of the buffer
    ids: it is part of the program (and of the workspace layout on the device)."""
    nk = len(hp["resblock_kernel_sizes"])
    c0 = hp["upsample_initial_channel"]
    wpre = _wt(sd, "conv_pre")
    x = nb.buf(c0, 1)
    nb.conv(L.BUF_INPUT, x, wpre.shape[1], c0, pack.pack_conv(wpre), sd["conv_pre.bias"], k=7, pad=3)
    tm, ch = 1, c0
    for i, (u, k) in enumerate(zip(hp["upsample_rates"], hp["upsample_kernel_sizes"])):
        cin, ch = c0 // (2 ** i), c0 // (2 ** (i + 1))
        tm *= u
        xu = nb.buf(ch, tm)
        nb.conv(x, xu, cin, ch, pack.pack_conv_transpose(_wt(sd, ups.format(i)), u), sd[ups.format(i) + ".bias"], tr_stride=u,
                tr_pad=(k - u) // 2, tr_k=k, **ups_act)
        nb.release(x)
        xs = nb.buf(ch, tm)
        for j, (rk, rd) in enumerate(zip(hp["resblock_kernel_sizes"], hp["resblock_dilation_sizes"])):
            r = xu
            for m, d in enumerate(rd):
                last = m == len(rd) - 1
                dst = xs if last else nb.buf(ch, tm)
                al, be = (1.0 / nk, 0.0 if j == 0 else 1.0) if last else (1.0, 0.0)
                step(f"resblocks.{i * nk + j}.", m, r, dst, ch, tm, rk, d, al, be)
                if r != xu:
                    nb.release(r)
                r = dst
        nb.release(xu)
        x = xs
    x, post_act = post(x, ch, tm)
    wpost = _wt(sd, "conv_post")
    nb.conv(x, L.BUF_OUTPUT, ch, wpost.shape[0], pack.pack_conv(wpost), sd["conv_post.bias"], k=7, pad=3, out_act=L.ACT_TANH, **post_act)
    return ConvNet(ctx, L.NET_VOCODER, nb, wpre.shape[1], wpost.shape[0], tm)


def build_hifigan(ctx: Context, sd: Dict[str, Tensor], hp: dict, precision: str = "split", fuse_pairs: Sequence[int] = (32, 64)) -> ConvNet:
    """HifiGanGenerator.forward (vocoder/hifigan/modules/hifigan.py:126-143) as an op list; fully
    driven by the vocoder's config.yaml keys."""
    nb = NetBuilder(ctx.device, precision)
    fp32_rule = nb.row.fp32_pairs is not None
    fp32_pairs = tuple(int(v) for v in _switch("VB_FP32_PAIRS", nb.row.fp32_pairs or "32,64").split(",") if v.strip())

    def step(p, m, r, dst, ch, tm, rk, d, al, be):
        # (fp32 pair kernel: 16-byte window DMA needs T % 4 == 0 - guaranteed for every mel length, chunked runs included, when the
        #  stage's length multiplier is a multiple of 4; other stages keep the two unfused launches)
        fuse = (ch in fp32_pairs and (rk - 1) * d <= 60 and rk <= 17 and tm % 4 == 0) if fp32_rule else (ch in fuse_pairs and (rk - 1) * d <= 64)
        if hp["resblock"] == "1" and fuse and rk % 2 == 1:
            # narrowest, longest stage: both convolutions of the pair in one launch, intermediate kept in LDS
            # (measured: 645 us per pair against 2 x 600 us at 32 channels; at 64 channels the fused kernel
            #  fits one workgroup per CU only and loses, 1525 us against 2 x 640 us - so it is not used there)
            nb.respair(r, dst, ch, *_wb(sd, f"{p}convs1.{m}"), *_wb(sd, f"{p}convs2.{m}"), rk, d, 0.1, al, be)
        elif hp["resblock"] == "1":
            t1 = nb.buf(ch, tm)
            # the LeakyReLU between the two convolutions is applied by the FIRST one's epilogue (t1 has no other reader), not by the
            # second one's window pass: the same values (max(v, 0.1 v) either way), one in-place LDS pass per 16-channel chunk less
            # in every second convolution (round 6)
            mid_out = not _switch("VB_LRELU_IN_WINDOW")
            nb.conv(r, t1, ch, ch, *_wb(sd, f"{p}convs1.{m}"), k=rk, dil=d, pad=(rk * d - d) // 2, in_act=L.ACT_LRELU, in_slope=0.1,
                    out_act=L.ACT_LRELU if mid_out else L.ACT_NONE, out_slope=0.1 if mid_out else 0.0)
            nb.conv(t1, dst, ch, ch, *_wb(sd, f"{p}convs2.{m}"), k=rk, pad=(rk - 1) // 2, in_act=L.ACT_NONE if mid_out else L.ACT_LRELU,
                    in_slope=0.0 if mid_out else 0.1, res=r, alpha=al, beta=be)
            nb.release(t1)
        else:
            nb.conv(r, dst, ch, ch, *_wb(sd, f"{p}convs.{m}"), k=rk, dil=d, pad=(rk * d - d) // 2, in_act=L.ACT_LRELU, in_slope=0.1, res=r,
                    alpha=al, beta=be)

    # differences from the shared walk: the upsampler sits at ups.{i} behind a LeakyReLU(0.1), conv_post behind a LeakyReLU(0.01)
    return _vocoder_walk(ctx, nb, sd, hp, "ups.{}", dict(in_act=L.ACT_LRELU, in_slope=0.1), step,
                         lambda x, ch, tm: (x, dict(in_act=L.ACT_LRELU, in_slope=0.01)))


def build_bigvgan(ctx: Context, sd: Dict[str, Tensor], hp: dict, precision: str = "split") -> ConvNet:
    """BigVGAN.forward (vocoder/bigvgan/models.py:181-205) as an op list: conv_pre, per stage ConvTranspose (no activation in
    front of it) + the mean of the AMP blocks (anti-aliased Snake/SnakeBeta -> conv -> ... + x), anti-aliased activation,
    conv_post, tanh.  Driven by the args.yml keys; weights are weight-norm pairs like the HiFi-GAN's."""
    nb = NetBuilder(ctx.device, precision)
    logscale = bool(hp["snake_logscale"])

    def act(name, x, ch, tm):
        out = nb.buf(ch, tm)
        nb.aa_act(x, out, ch, sd[name + ".act.alpha"], sd.get(name + ".act.beta"), logscale)
        return out

    def step(p, m, r, dst, ch, tm, rk, d, al, be):
        if hp["resblock"] == "1":
            a1 = act(f"{p}activations.{2 * m}", r, ch, tm)
            t1 = nb.buf(ch, tm)
            nb.conv(a1, t1, ch, ch, *_wb(sd, f"{p}convs1.{m}"), k=rk, dil=d, pad=(rk * d - d) // 2)
            nb.release(a1)
            a2 = act(f"{p}activations.{2 * m + 1}", t1, ch, tm)
            nb.release(t1)
            nb.conv(a2, dst, ch, ch, *_wb(sd, f"{p}convs2.{m}"), k=rk, pad=(rk - 1) // 2, res=r, alpha=al, beta=be)
            nb.release(a2)
        else:
            a1 = act(f"{p}activations.{m}", r, ch, tm)
            nb.conv(a1, dst, ch, ch, *_wb(sd, f"{p}convs.{m}"), k=rk, dil=d, pad=(rk * d - d) // 2, res=r, alpha=al, beta=be)
            nb.release(a1)

    # differences from the shared walk: the upsampler sits at ups.{i}.0 with no activation, conv_post behind an anti-aliased activation
    return _vocoder_walk(ctx, nb, sd, hp, "ups.{}.0", {}, step, lambda x, ch, tm: (act("activation_post", x, ch, tm), {}))
