"""Host-side mirror of the reference's operator API for the inference path.

Same class names, constructor params (configs/vocal2music.yaml), method names,
argument meaning and error behaviour as the reference modules they stand in for,
so ``scripts/test_final.py``-style callers run unchanged; the compute underneath
is libversband_hip.so (versband_amd.engine).  The ``ldm.*`` / ``vocoder.*``
packages at the repo root re-export these under the reference's dotted paths so
``instantiate_from_config`` resolves the YAML ``target`` strings as-is.
"""
from __future__ import annotations

import glob
import importlib
import os
import re
import warnings
from typing import Any, Dict, List, Optional

import numpy as np
import torch
import yaml

from . import prng
from .synth import DiTConfig, HifiGanConfig, VAEConfig

Tensor = torch.Tensor

# ---------------------------------------------------------------------------
# config / factory  (ldm/util.py:110-125, OmegaConf stand-in)
# ---------------------------------------------------------------------------


class AttrDict(dict):
    """dict with attribute access, enough of OmegaConf's DictConfig for this path."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    @staticmethod
    def wrap(o):
        if isinstance(o, dict):
            return AttrDict({k: AttrDict.wrap(v) for k, v in o.items()})
        if isinstance(o, list):
            return [AttrDict.wrap(v) for v in o]
        return o


def load_config(path: str) -> AttrDict:
    with open(path) as f:
        return AttrDict.wrap(yaml.safe_load(f))


def get_obj_from_str(string: str, reload: bool = False):
    module, cls = string.rsplit(".", 1)
    m = importlib.import_module(module)
    if reload:
        importlib.reload(m)
    return getattr(m, cls)


def instantiate_from_config(config, reload: bool = False):
    """ldm/util.py:110-117: ``target`` dotted path + ``params`` kwargs."""
    if "target" not in config:
        if config == "__is_first_stage__" or config == "__is_unconditional__":
            return None
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(config["target"], reload=reload)(**config.get("params", dict()))


# ---------------------------------------------------------------------------
# network holders
# ---------------------------------------------------------------------------


class TxtFlagLargeImprovedDiTV2:
    """Parameter holder for vocal2music_moe.py:477-520 (same ctor signature)."""

    def __init__(self, in_channels, context_dim, hidden_size=1152, depth=28, num_heads=16, max_len=1000, num_experts=4,
                 ori_dim=1024):
        # ori_dim is accepted and ignored exactly like the reference ctor: T5 width stays 1024
        self.cfg = DiTConfig(in_channels=in_channels, ori_dim=1024, context_dim=context_dim, hidden_size=hidden_size,
                             num_heads=num_heads, depth=depth, max_len=max_len, num_experts=num_experts)
        if context_dim != hidden_size:
            raise ValueError("context_dim must equal hidden_size (cap_embedder / Attention y_dim, vocal2music_moe.py:367-373)")
        self.in_channels = self.out_channels = in_channels


class AutoencoderKL:
    """ldm/models/autoencoder1d.py:14-58 (decode side)."""

    def __init__(self, embed_dim, ddconfig, lossconfig=None, ckpt_path=None, ignore_keys=(), image_key="image", monitor=None):
        assert ddconfig["double_z"]
        self.embed_dim = embed_dim
        self.ddconfig = dict(ddconfig)
        self.image_key = image_key
        self.state: Dict[str, Tensor] = {}
        self.net = None
        if ckpt_path is not None:
            if os.path.exists(ckpt_path):
                self.init_from_ckpt(ckpt_path, ignore_keys)
            else:
                warnings.warn(f"AutoencoderKL ckpt_path {ckpt_path} not found; weights must come from the CFM checkpoint")

    def init_from_ckpt(self, path, ignore_keys=()):
        sd = torch.load(path, map_location="cpu")["state_dict"]
        sd = {k: v for k, v in sd.items() if not any(k.startswith(ik) for ik in ignore_keys)}
        self.load_state_dict(sd)

    def load_state_dict(self, sd, strict=False):
        self.state = {k: v for k, v in sd.items() if k.startswith("decoder.") or k.startswith("post_quant_conv.")}
        self.enc_state = {k: v for k, v in sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}
        self.net = None
        self.enc_net = None

    enc_state: Dict[str, Tensor] = {}
    enc_net = None
    _device = None
    _precision = "fp32mf"        # VAE arithmetic: fp32 with minimal filtering (default), "fp32" = direct fp32 kernels, "split" = bf16x3, "bf16" = single-pass bf16, "bf16xt" = the same with the wide layers as one-plane DMA-fed GEMMs (set by CFM(vocoder_precision=...))

    def encode(self, x, lengths=None):
        """:49-53  mel [B,80,T_mel] -> DiagonalGaussianDistribution over z [B,embed_dim,T_mel/2] (HIP encoder net).
        lengths (addition; ConvNet.encode_lens): one length in LATENT tokens per row - mels of different lengths padded to T_mel share the
        call, row b owns its first 2 * lengths[b] frames and the moments of row b are those of the clip alone followed by zeros (mean 0,
        logvar 0 behind the row's end: CFM.get_first_stage_encoding(..., lengths=) ends the sample there too)."""
        from .engine import Context, build_vae_encoder
        if self.enc_net is None:
            if not self.enc_state:
                raise RuntimeError("AutoencoderKL.encode: no encoder.* / quant_conv.* weights loaded")
            self.enc_net = build_vae_encoder(Context(self._device or "cuda:0"), self.enc_state, precision=self._precision)
        if lengths is not None:
            return DiagonalGaussianDistribution(self.enc_net.encode_lens(x, lengths))
        return DiagonalGaussianDistribution(self.enc_net.run(x))


class DiagonalGaussianDistribution:
    """ldm/modules/distributions/distributions.py:4-43 (inference members)."""

    def __init__(self, parameters: Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self, noise: Optional[Tensor] = None):
        eps = torch.randn(self.mean.shape, device=self.mean.device) if noise is None else noise.to(self.mean.device)
        return self.mean + self.std * eps

    def mode(self):
        return self.mean


class DiffusionWrapper:
    """ldm/models/diffusion/ddpm.py:1396-1446 ('hybrid' conditioning only)."""

    def __init__(self, diff_model_config, conditioning_key):
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        assert conditioning_key in (None, "concat", "crossattn", "hybrid", "adm", "film")


class FrozenTextVocalEmbedder:
    """ldm/modules/encoders/modules.py:194-233 boundary: returns {'caption': [B,L,1024] f32, 'acoustic', 'name'}.
    Captions given as pre-computed embeddings pass through; token ids run the T5 encoder stack on the HIP library; strings
    are tokenized (the sentencepiece tokenizer under `version`) and encoded like the reference does (modules.py:216-221).
    When strings arrive and the T5 weights or the tokenizer are missing this RAISES - the reference would have failed in
    from_pretrained(version) too.  Seeded stand-in embeddings for strings (BASELINE's "dummy T5 emb") are an explicit
    opt-in: `dummy_text=True` in the cond_stage_config params (scripts/test_final.py --dummy_text)."""

    def __init__(self, version="google/flan-t5-large", device="cuda", max_length=77, freeze=True, dummy_text=False, **kw):
        self.version, self.max_length, self.device = version, max_length, device
        self.dummy_text = bool(dummy_text)
        self.width = 1024
        self.t5_state: Dict[str, Tensor] = {}
        self.t5_heads, self.t5_eps = 16, 1e-6           # flan-t5-large / t5-v1_1-large encoder
        self._t5 = None
        self._tokenizer = None

    def to(self, device):
        self.device = device
        return self

    def load_state_dict(self, sd, strict=False):
        """`transformer.*` weights of the reference's cond_stage_model (HF T5EncoderModel keys, prefix already stripped)."""
        self.t5_state = {k: v for k, v in sd.items() if k.startswith("encoder.") or k == "shared.weight"}
        self._t5 = None

    def _t5_engine(self):
        from .engine import Context, T5Engine
        if self._t5 is None:
            dev = self.device if str(self.device).startswith("cuda:") else f"cuda:{torch.cuda.current_device()}"
            self._t5 = T5Engine(Context(dev), self.t5_state, num_heads=self.t5_heads, eps=self.t5_eps)
        return self._t5

    def _tokenize(self, caps: List[str]) -> Optional[Tensor]:
        """The tokenizer is upstream of the library; it is used when the checkpoint directory named by `version` is on disk."""
        if self._tokenizer is None:
            # `version` is a path relative to where the reference is launched from (useful_ckpts/flan-t5-large): try the cwd,
            # then the repository root
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            for cand in (self.version, os.path.join(root, self.version)):
                if os.path.isdir(cand):
                    from transformers import T5Tokenizer
                    self._tokenizer = T5Tokenizer.from_pretrained(cand)
                    break
        if self._tokenizer is None:
            return None
        enc = self._tokenizer(text=caps, truncation=True, max_length=self.max_length, return_length=True, return_overflowing_tokens=False,
                              padding="max_length", return_tensors="pt")
        return enc["input_ids"]

    def _embed_text(self, caps: List[str]) -> Tensor:
        out = []
        for c in caps:
            ks = prng.key_seed(20240921, "t5:" + c)
            out.append(torch.from_numpy(prng.normal(ks, self.max_length * self.width).reshape(self.max_length, self.width)))
        return torch.stack(out)

    def encode(self, c):
        return self(c)

    def __call__(self, c):
        cap = c["caption"]
        if torch.is_tensor(cap) and cap.dtype in (torch.int64, torch.int32) and cap.dim() == 2:
            # token ids [B, L]: run the T5 encoder stack on the HIP library (modules.py:216-221 without the tokenizer)
            if not self.t5_state:
                raise RuntimeError("FrozenTextVocalEmbedder: token ids given but no cond_stage_model.transformer.* weights loaded")
            cap = self._t5_engine().encode(cap)
        elif not torch.is_tensor(cap):
            ids = self._tokenize(list(cap)) if self.t5_state else None
            if ids is not None:
                cap = self._t5_engine().encode(ids)
            elif self.dummy_text:
                cap = self._embed_text(list(cap))
            else:
                what = "no cond_stage_model.transformer.* weights are loaded" if not self.t5_state else \
                    f"the tokenizer directory {self.version!r} does not exist"
                raise RuntimeError(f"FrozenTextVocalEmbedder: text captions given but {what}; pass pre-computed T5 embeddings / token "
                                   "ids, load a checkpoint with the T5 encoder, or opt in to seeded stand-in embeddings with dummy_text=True")
        return {"caption": cap.float(), "acoustic": c["acoustic"], "name": c.get("name")}


# ---------------------------------------------------------------------------
# CFM model shell  (ldm/models/diffusion/cfm1_audio.py:31-36 over ddpm_audio.py LatentDiffusion_audio)
# ---------------------------------------------------------------------------


class CFM:
    def __init__(self, unet_config=None, first_stage_config=None, cond_stage_config=None, timesteps=1000, mel_dim=80,
                 mel_length=848, channels=0, conditioning_key=None, scale_by_std=False, scale_factor=1.0, precision="bf16",
                 vocoder_precision="fp32mf", **ignored):
        # precision: the DiT ("bf16" production / "split" = bf16x3 parity mode).  vocoder_precision: the first-stage VAE ("fp32" = the
        # reference's arithmetic on the f32 MFMA, direct kernels; "fp32mf" = the same with F(2,3) minimal filtering on the 3-tap layers, the default since
    # round 6; "split" = bf16x3, <= 3e-5 of it and 1.2x faster end to end)
        self.num_timesteps = timesteps
        self.mel_dim, self.mel_length, self.channels = mel_dim, mel_length, channels
        self.sigma_min = 1e-4
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        self.first_stage_model = instantiate_from_config(first_stage_config)
        self.cond_stage_model = instantiate_from_config(cond_stage_config)
        self.cond_stage_forward = None
        self.scale_factor = torch.tensor(float(scale_factor))
        self.precision = precision
        assert vocoder_precision in ("fp32", "split", "fp32mf", "bf16", "bf16xt"), vocoder_precision
        self.vocoder_precision = vocoder_precision
        self.first_stage_model._precision = vocoder_precision
        self.device = torch.device("cpu")
        self._dit_state: Dict[str, Tensor] = {}
        self._ctx = None
        self._dit = None
        self._cond_cache: Dict[int, Any] = {}
        self._nfe = 0                     # apply_model calls so far: keys the on-device router noise of each call

    # -- checkpoint (scripts/test_final.py:143) ----------------------------
    def load_state_dict(self, sd: Dict[str, Tensor], strict: bool = False):
        dp, fp = "model.diffusion_model.", "first_stage_model."
        dit = {k[len(dp):]: v for k, v in sd.items() if k.startswith(dp)}
        if dit:
            self._dit_state = dit
            self._dit = None
        vae = {k[len(fp):]: v for k, v in sd.items() if k.startswith(fp)}
        if vae:
            self.first_stage_model.load_state_dict(vae)
        cp = "cond_stage_model.transformer."
        t5 = {k[len(cp):]: v for k, v in sd.items() if k.startswith(cp)}
        if t5 and hasattr(self.cond_stage_model, "load_state_dict"):
            self.cond_stage_model.load_state_dict(t5)
        if "scale_factor" in sd:
            self.scale_factor = sd["scale_factor"].detach().float().cpu().reshape(())
        if strict:
            from .synth import dit_shapes
            missing = [k for k in dit_shapes(self.model.diffusion_model.cfg) if k not in dit]
            if missing:
                raise RuntimeError(f"Missing key(s) in state_dict: {missing[:5]} ...")
        return [], []

    def eval(self):
        return self

    def to(self, device):
        self.device = torch.device(device)
        if hasattr(self.cond_stage_model, "to"):
            self.cond_stage_model.to(self.device)        # the reference does cond_stage_model.to(model.device): one GPU per process
        return self

    # -- engines -----------------------------------------------------------
    def _context(self):
        from .engine import Context
        if self._ctx is None or self._ctx.device != self.device:
            self._ctx = Context(self.device)
            self._dit = None
            self.first_stage_model.net = None
        return self._ctx

    def dit_engine(self):
        from .engine import DiTEngine
        ctx = self._context()
        if self._dit is None:
            if not self._dit_state:
                raise RuntimeError("CFM: no DiT weights loaded (load_state_dict first)")
            self._dit = DiTEngine(ctx, self.model.diffusion_model.cfg, self._dit_state, precision=self.precision)
        return self._dit

    def vae_net(self):
        from .engine import build_vae_decoder
        ctx = self._context()
        fs = self.first_stage_model
        if fs.net is None:
            if not fs.state:
                raise RuntimeError("CFM: no first_stage_model weights loaded")
            fs.net = build_vae_decoder(ctx, fs.state, scale_factor=float(self.scale_factor), precision=self.vocoder_precision)
        return fs.net

    # -- reference API -----------------------------------------------------
    def get_learned_conditioning(self, c):
        """ddpm_audio.py:182-193."""
        if hasattr(self.cond_stage_model, "encode") and callable(self.cond_stage_model.encode):
            return self.cond_stage_model.encode(c)
        return self.cond_stage_model(c)

    def _precompute(self, conds: List[dict], T: int, lengths=None):
        def sig(t):       # identity AND content version of a tensor: an in-place edit or a swapped tensor invalidates the entry
            return (t.data_ptr(), t._version, tuple(t.shape)) if torch.is_tensor(t) else id(t)
        key = tuple((id(c), sig(c["caption"]), sig(c["acoustic"].get("midi")), sig(c["acoustic"].get("beats"))) for c in conds) + (T, None if lengths is None else tuple(int(v) for v in lengths))
        hit = self._cond_cache.get(key)
        if hit is not None:
            return hit[0]
        ac = conds[0]["acoustic"]
        t5 = torch.cat([c["caption"].float().to(self.device) for c in conds], dim=0)
        pc = self.dit_engine().precompute_cond(t5, ac["midi"], ac["beats"], T, **({} if lengths is None else {"lengths": lengths}))
        self._cond_cache = {key: (pc, conds)}     # single entry: holds the cond dicts alive so ids stay unique
        return pc

    @torch.no_grad()
    def apply_model(self, x_noisy, t, cond, return_ids=False):
        """ddpm_audio.py:443-469: one conditional evaluation -> (v, lb_loss)."""
        if not isinstance(cond, dict):
            raise NotImplementedError("only the hybrid dict conditioning of configs/vocal2music.yaml is supported")
        pc = self._precompute([cond], x_noisy.shape[-1])
        # every call draws fresh Gumbel router noise like the reference's gumbel_softmax does: the counter-based draws are keyed
        # by (seed, clip, evaluation index, block, gate), so the evaluation index advances per call
        v = self.dit_engine().forward(x_noisy, t, pc, seed=int(torch.initial_seed()) & 0xFFFFFFFF, nfe=self._nfe)
        self._nfe += 1
        # lb_loss (vocal2music_moe.py:427-429) is a training-only auxiliary; the inference callers discard it
        return v, torch.zeros((), device=v.device)

    @torch.no_grad()
    def encode_first_stage(self, x, lengths=None):
        """ddpm_audio.py:411-412.
        lengths (addition; ConvNet.encode_lens): one length in latent tokens per row, the unit of sample_cfg(lengths=) and
        decode_first_stage(lengths=) - mels of different lengths padded to x.shape[-1] share the call."""
        self.first_stage_model._device = self._context().device
        if lengths is not None:
            return self.first_stage_model.encode(x, lengths=lengths)
        return self.first_stage_model.encode(x)

    def get_first_stage_encoding(self, encoder_posterior, lengths=None, noise=None, mode=False):
        """ddpm_audio.py:163-170.
        lengths (addition; vb_posterior_lens): the posterior of encode_first_stage(x, lengths=) - or its moments [B, 2E, T] - sampled and
        scaled in one launch, row b's latent exactly zero from lengths[b] on (what sample_cfg(x_known=, lengths=) expects of a padded
        latent; the elementwise path leaves the noise there, the moments' zero tail being std = 1).  noise: the draw [B, E, T] to use,
        None = torch.randn on the device as DiagonalGaussianDistribution.sample does; mode = True: the mean, no draw.  Without lengths
        the reference path, unchanged (noise and mode are then not read)."""
        if lengths is not None:
            return self._posterior_lens(encoder_posterior, lengths, noise, mode)
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample()
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return float(self.scale_factor) * z

    def _posterior_lens(self, encoder_posterior, lengths, noise, mode) -> Tensor:
        from . import _lib as L
        from .engine import _lens_struct
        mom = encoder_posterior.parameters if isinstance(encoder_posterior, DiagonalGaussianDistribution) else encoder_posterior
        if not isinstance(mom, torch.Tensor) or mom.dim() != 3 or mom.shape[1] % 2:
            raise ValueError("get_first_stage_encoding(lengths=): a DiagonalGaussianDistribution or its moments [B, 2E, T]")
        dev = self._context().device
        mom = mom.to(dev, torch.float32).contiguous()
        B, E, T = mom.shape[0], mom.shape[1] // 2, mom.shape[2]
        lens, hold, _ = _lens_struct(lengths, B, T, gloss=" (latent tokens per row)")
        eps = None
        if not mode:
            eps = torch.randn(B, E, T, device=dev) if noise is None else noise.to(dev, torch.float32).contiguous()
            if tuple(eps.shape) != (B, E, T):
                raise ValueError(f"get_first_stage_encoding: noise of shape {tuple(eps.shape)}, not {(B, E, T)}")
        z = torch.empty(B, E, T, dtype=torch.float32, device=dev)
        L.check(self._context().lib.vb_posterior_lens(L.ptr(mom), L.ptr(eps) if eps is not None else None, B, E, T, lens.len if lens is not None else None,
                                                     float(self.scale_factor), L.ptr(z), L.stream_ptr()), "vb_posterior_lens")
        del hold
        return z

    @torch.no_grad()
    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False, lengths=None):
        """ddpm_audio.py:379-392: z / scale_factor -> AutoencoderKL.decode.
        lengths (addition; ConvNet.decode_lens): one length in latent tokens per row - latents of different lengths padded to T share the
        call, row b holds 2 * lengths[b] mel frames of the clip alone followed by zeros, the latent padding is never read."""
        if lengths is not None:
            return self.vae_net().decode_lens(z, lengths)
        return self.vae_net().run(z)


# ---------------------------------------------------------------------------
# sampler  (ldm/models/diffusion/cfm1_audio_sampler.py)
# ---------------------------------------------------------------------------


def euler_tables(timesteps: int, t_start: Optional[int] = None):
    """t_span = linspace(0,1,timesteps) (:108), optional t_span[t_start:] (:110-111); per step the solver's dt
    (float32, accumulated like torchdyn's fixed-step loop) and the integer index Wrapper_cfg feeds the DiT:
    trunc(float32(t)*1000) (cfm1_audio.py:156 - SURVEY Q3)."""
    t_span = torch.linspace(0, 1, timesteps)
    if t_start is not None:
        t_span = t_span[t_start:]
    idx, dts = [], []
    t = t_span[0]
    for k in range(len(t_span) - 1):
        dt = t_span[k + 1] - t
        idx.append(int(torch.tensor([t * 1000]).long().item()))
        dts.append(float(dt))
        t = t + dt
    return idx, dts


def euler_times(timesteps: int, t_start: Optional[int] = None) -> List[float]:
    """the time after each step of euler_tables(timesteps, t_start): float32, accumulated t += dt like the solver loop does (the
    table a known-region call hands to vb_sample_cfg_keep as t_next)"""
    t_span = torch.linspace(0, 1, timesteps)
    if t_start is not None:
        t_span = t_span[t_start:]
    out = []
    t = t_span[0]
    for k in range(len(t_span) - 1):
        dt = t_span[k + 1] - t
        t = t + dt
        out.append(float(t))
    return out


def guidance_interval_weights(timesteps: int, lo: float, hi: float, t_start: Optional[int] = None) -> List[float]:
    """per-step guidance weights of a guidance interval on the grid of euler_tables(timesteps, t_start): 1.0 where the step's start time
    t_span[k] lies in [lo, hi] (both ends included, compared in float32 like the grid), 0.0 elsewhere - the step is then a plain
    conditional one (DiTEngine.sample_cfg(guidance=...))."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError(f"guidance interval [{lo}, {hi}]: two finite values lo <= hi")
    t_span = torch.linspace(0, 1, timesteps)
    if t_start is not None:
        t_span = t_span[t_start:]
    lo32, hi32 = np.float32(lo), np.float32(hi)
    return [1.0 if lo32 <= np.float32(t) <= hi32 else 0.0 for t in t_span[:-1].tolist()]


def guidance_arg(guidance_weights, guidance_interval, timesteps: int, t_start: Optional[int] = None):
    """the guidance arguments of CFMSampler.sample_cfg -> the `guidance` list of DiTEngine.sample_cfg, or None for the plain call (neither
    given, or every weight 1).  At most one of the two; the weights are n finite numbers in [0, 16], the interval is (lo, hi)."""
    if guidance_weights is not None and guidance_interval is not None:
        raise ValueError("guidance_weights and guidance_interval do not go together: give at most one")
    if guidance_interval is not None:
        try:
            lo, hi = guidance_interval
        except (TypeError, ValueError):
            raise ValueError("guidance_interval must be (lo, hi)") from None
        w = guidance_interval_weights(timesteps, lo, hi, t_start)
    elif guidance_weights is not None:
        n = len(euler_tables(timesteps, t_start)[0])
        w = guidance_weights.tolist() if torch.is_tensor(guidance_weights) else list(guidance_weights)
        if any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) for v in w):
            raise TypeError("guidance_weights must hold numbers (one weight per step)")
        if len(w) != n:
            raise ValueError(f"guidance_weights has {len(w)} entries for {n} steps")
        w = [float(v) for v in w]
        for k, v in enumerate(w):
            if not (np.isfinite(v) and 0.0 <= v <= 16.0):
                raise ValueError(f"guidance_weights[{k}] = {v} is not a finite value in [0, 16]")
    else:
        return None
    return None if all(v == 1.0 for v in w) else w


def keep_block(x_known, keep_mask, keep_noise, x_latent, t_start, shape, timesteps, sigma_min):
    """the known-region arguments of CFMSampler.sample_cfg -> the (ref, x0, mask, t_next, sigma_min) block of DiTEngine.sample_cfg, or None
    when no region is given.  x_known is in the sampler's latent scale; keep_mask [B,T] or [T]; keep_noise is the start noise of the
    path the known tokens are held on: x_latent when the call starts from the noise (t_start is None), required otherwise."""
    if x_known is None and keep_mask is None:
        if keep_noise is not None:
            raise ValueError("keep_noise without x_known / keep_mask")
        return None
    if x_known is None or keep_mask is None:
        raise ValueError("x_known and keep_mask go together")
    if keep_noise is None:
        if t_start is not None:
            raise ValueError("keep_noise is required with t_start: the state the call starts from is not the noise the known region's "
                             "path is built on (nothing is re-drawn silently)")
        if x_latent is None:
            raise ValueError("keep_noise (or x_latent, the start noise) is required with x_known")
        keep_noise = x_latent
    B, _, T = shape
    if tuple(x_known.shape) != tuple(shape):
        raise ValueError(f"x_known has shape {tuple(x_known.shape)}, expected {tuple(shape)}")
    if tuple(keep_noise.shape) != tuple(shape):
        raise ValueError(f"keep_noise has shape {tuple(keep_noise.shape)}, expected {tuple(shape)}")
    mask = keep_mask.to(torch.float32)
    if mask.dim() == 1:
        mask = mask.unsqueeze(0).expand(B, -1)
    if tuple(mask.shape) != (B, T):
        raise ValueError(f"keep_mask has shape {tuple(keep_mask.shape)}, expected ({B}, {T}) or ({T},)")
    if mask.numel() and (float(mask.min()) < 0.0 or float(mask.max()) > 1.0 or bool(torch.isnan(mask).any())):
        raise ValueError("keep_mask values must lie in [0, 1]")
    return (x_known.to(torch.float32).contiguous(), keep_noise.to(torch.float32).contiguous(), mask.contiguous(),
            euler_times(timesteps, t_start), float(sigma_min))


class CFMSampler(object):
    def __init__(self, model, num_timesteps, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.num_timesteps = num_timesteps
        self.schedule = schedule

    def stochastic_encode(self, x_start, t, noise=None):
        """:41-46."""
        x0 = torch.randn_like(x_start) if noise is None else noise
        tu = 1 - t.unsqueeze(1).unsqueeze(1).float() / self.num_timesteps
        return tu * x_start + (1.0 - (1 - self.model.sigma_min) * tu) * x0

    def _shape(self, shape, batch_size):
        if shape is None:
            if self.model.channels > 0:
                shape = (batch_size, self.model.channels, self.model.mel_dim, self.model.mel_length)
            else:
                shape = (batch_size, self.model.mel_dim, self.model.mel_length)
            return tuple(shape)
        if len(shape) == 3:
            raise NotImplementedError("2-D latents are not part of the vocal2music path")
        C, T = shape
        return (batch_size, C, T)

    @torch.no_grad()
    def sample_cfg(self, cond, unconditional_guidance_scale, unconditional_conditioning, batch_size=16, timesteps=None, shape=None,
                   x_latent=None, t_start=None, gumbel_noise=None, seed=None, clip_base=0, x_known=None, keep_mask=None, keep_noise=None,
                   clip_ids=None, *, guidance_weights=None, guidance_interval=None, lengths=None, **kwargs):
        """:87-116.  Extra kwargs (S=, x_T=, verbose=) are tolerated and ignored like the reference does
        (SURVEY Q1/Q2).  gumbel_noise/seed/clip_base are additions: injected router noise for parity, or the
        (seed, global clip index) that keys the on-device counter-based draws.
        x_known / keep_mask / keep_noise (addition; inpainting, continuation): tokens where keep_mask [B,T] or [T] is 1 are held on the
        probability path from keep_noise to x_known (the sampler's latent scale, what get_first_stage_encoding returns) and end at
        x_known + sigma_min * keep_noise; the others are generated in agreement with them.  keep_noise defaults to the start noise
        when t_start is None and is required with t_start.
        unconditional_guidance_scale may hold one value per row (sequence / float32 tensor) and clip_ids one global clip index per row
        (addition; DiTEngine.sample_cfg): rows of different scales or non-contiguous clips then share the call.
        guidance_weights (one weight in [0, 16] per step) or guidance_interval = (lo, hi) (addition, keyword-only, at most one of them):
        step k runs under the effective scale 1 + w_k (scale - 1); the interval is w_k = 1 where the step starts at t in [lo, hi] and 0
        elsewhere, and a step of weight 0 evaluates the conditional branch alone.
        lengths (addition, keyword-only; DiTEngine.sample_cfg): one length in latent tokens per row - clips of different lengths padded
        to shape[-1] share the call, row b's first lengths[b] tokens are the call on that clip alone (midi / beats hold 2 * shape[-1]
        frames per row, those beyond 2 * lengths[b] are not read), the padding of the result is zero."""
        shape = self._shape(shape, batch_size)
        timesteps = 25 if timesteps is None else timesteps
        idx, dts = euler_tables(timesteps, t_start)
        guidance = guidance_arg(guidance_weights, guidance_interval, timesteps, t_start)
        dev = self.model.device
        x0 = torch.randn(shape, device=dev) if x_latent is None else x_latent
        keep = keep_block(x_known, keep_mask, keep_noise, x0, t_start, shape, timesteps, self.model.sigma_min)
        conds = [cond] if unconditional_conditioning is None else [cond, unconditional_conditioning]
        pc = self.model._precompute(conds, shape[-1], **({} if lengths is None else {"lengths": lengths}))
        if seed is None:
            seed = int(torch.initial_seed()) & 0xFFFFFFFF
        scale = unconditional_guidance_scale
        if isinstance(scale, (int, float, np.integer, np.floating)) and not isinstance(scale, bool):
            scale = float(scale)
        x, traj = self.model.dit_engine().sample_cfg(x0, pc, idx, dts, scale, noise=gumbel_noise,
                                                     seed=seed, clip_base=clip_base, return_traj=True, keep=keep, clip_ids=clip_ids,
                                                     **({} if guidance is None else {"guidance": guidance}),
                                                     **({} if lengths is None else {"lengths": lengths}))
        return traj[-1], traj

    @torch.no_grad()
    def sample(self, cond, batch_size=16, timesteps=None, shape=None, x_latent=None, t_start=None, x_known=None, keep_mask=None,
               keep_noise=None, clip_ids=None, **kwargs):
        """:49-80 (no guidance).  (lengths= travels in kwargs, as in sample_cfg.)"""
        return self.sample_cfg(cond, 1.0, None, batch_size=batch_size, timesteps=timesteps, shape=shape, x_latent=x_latent,
                               t_start=t_start, x_known=x_known, keep_mask=keep_mask, keep_noise=keep_noise, clip_ids=clip_ids, **kwargs)


# ---------------------------------------------------------------------------
# vocoder  (vocoder/hifigan/hifigan.py:7-43, utils/commons/{hparams,ckpt_utils}.py)
# ---------------------------------------------------------------------------


def set_hparams(config_path: str) -> dict:
    """utils/commons/hparams.py:25-133 reduced to what HifiGAN needs: yaml + base_config inheritance."""
    def load(p, seen):
        with open(p) as f:
            hp = yaml.safe_load(f) or {}
        out = {}
        bases = hp.get("base_config", [])
        if isinstance(bases, str):
            bases = [bases]
        for b in bases:
            if b.startswith("."):
                b = os.path.normpath(os.path.join(os.path.dirname(p), b))
            if b not in seen and os.path.exists(b):
                out.update(load(b, seen | {b}))
        out.update({k: v for k, v in hp.items() if k != "base_config"})
        return out
    return load(config_path, {config_path})


def load_ckpt_state(ckpt_base_dir: str, model_name: str = "model_gen") -> Dict[str, Tensor]:
    """utils/commons/ckpt_utils.py:7-67: newest model_ckpt_steps_N.ckpt, state_dict[model_name] or 'model_name.'-prefixed keys."""
    if os.path.isfile(ckpt_base_dir):
        path = ckpt_base_dir
    else:
        paths = sorted(glob.glob(f"{ckpt_base_dir}/model_ckpt_steps_*.ckpt"),
                       key=lambda x: -int(re.findall(r".*steps\_(\d+)\.ckpt", x)[0]))
        assert len(paths) > 0, f"| ckpt not found in {ckpt_base_dir}."
        path = paths[0]
    sd = torch.load(path, map_location="cpu")["state_dict"]
    if len([k for k in sd.keys() if "." in k]) > 0:
        sd = {k[len(model_name) + 1:]: v for k, v in sd.items() if k.startswith(f"{model_name}.")}
    else:
        sd = sd[model_name]
    return sd


class HifiGAN:
    def __init__(self, vocoder_ckpt, device=None, precision="fp32mf"):
        """vocoder/hifigan/hifigan.py:7-18.  precision: "fp32mf" (default since round 6) = the reference's fp32 arithmetic on the f32 MFMA with
        F(2,3) minimal filtering on the ResBlock convolutions (fp32 products, fewer of them; same bounds against the reference's outputs as
        "fp32" = the direct fp32 kernels); "split" = bf16x3 (<= 3e-5 of it, faster); "bf16" = one bf16 pass per convolution (RN-bf16 weights
        x RN-bf16 activations, fp32 accumulation: a preview / draft mode outside the 1e-3 parity contract); "bf16xt" =
        the same arithmetic, wide layers reading a pre-activated bf16 plane by DMA (no layer of the default HiFi-GAN is that wide)"""
        assert precision in ("fp32", "split", "fp32mf", "bf16", "bf16xt"), precision
        self.precision = precision
        base_dir = vocoder_ckpt
        self.config = set_hparams(f"{base_dir}/config.yaml")
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.state = load_ckpt_state(base_dir, "model_gen")
        self._net = None
        self._ctx = None

    @classmethod
    def from_state(cls, config: dict, state: dict, device=None, precision="fp32mf") -> "HifiGAN":
        """the generator from an already loaded config + `model_gen` state dict (multi-GPU runs: rank 0 reads <vocoder_ckpt> and the
        weights reach the other ranks through versband_amd.dist.broadcast_state instead of N disk reads)"""
        self = cls.__new__(cls)
        self.precision = precision
        self.config = dict(config)
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.state = state
        self._net = None
        self._ctx = None
        return self

    def net(self):
        from .engine import Context, build_hifigan
        if self._net is None:
            self._ctx = Context(self.device)
            self._net = build_hifigan(self._ctx, self.state, self.config, precision=self.precision)
        return self._net

    def spec2wav(self, mel, **kwargs):
        """mel [T,80] (numpy / cpu tensor) -> wav float32 numpy [T*hop]  (hifigan.py:20-30)."""
        c = torch.as_tensor(np.asarray(mel) if not torch.is_tensor(mel) else mel, dtype=torch.float32).unsqueeze(0)
        c = c.transpose(2, 1).contiguous()
        return self.net().run(c).view(-1).cpu().numpy()

    def spec2wav_batch(self, mel_bct: Tensor, lengths=None, chunk=None, halo: int = 32) -> Tensor:
        """device-resident batched path: mel [B,80,T] -> wav [B, T*hop] (no host round trip).
        lengths (addition; ConvNet.run): one length in mel frames per row - mels of different lengths padded to T share the call, row b
        holds lengths[b] * hop samples of the clip alone followed by zeros, the mel padding is never read.
        chunk (addition; longform.vocode_chunked): long mels in chunks of `chunk` frames with `halo` frames of context on both sides,
        with or without lengths; None is the whole-row call."""
        if chunk is not None:
            from . import longform
            return longform.vocode_chunked(self.net(), mel_bct, chunk, halo, lengths=lengths).squeeze(1)
        return self.net().run(mel_bct, **({} if lengths is None else {"lengths": lengths})).squeeze(1)

    def __call__(self, mel):
        return self.spec2wav(mel)

    def vocode(self, mel):
        assert len(mel.shape) == 2
        c = torch.as_tensor(np.asarray(mel) if not torch.is_tensor(mel) else mel, dtype=torch.float32).unsqueeze(0)
        if c.shape[1] != 80:
            c = c.transpose(2, 1)
        return self.net().run(c.contiguous()).view(-1).cpu().numpy()


class VocoderBigVGAN:
    """vocoder/bigvgan/models.py:393-414: <ckpt_vocoder>/best_netG.pt ['generator'] + <ckpt_vocoder>/args.yml -> BigVGAN generator
    on the HIP library (engine.build_bigvgan)."""

    def __init__(self, ckpt_vocoder, device="cuda", precision="fp32"):
        import yaml
        assert precision in ("fp32", "split", "fp32mf", "bf16", "bf16xt"), precision
        self.precision = precision
        sd = torch.load(os.path.join(ckpt_vocoder, "best_netG.pt"), map_location="cpu")
        self.state = {k: v for k, v in sd["generator"].items() if not k.endswith("filter")}     # the filters are recomputed
        with open(os.path.join(ckpt_vocoder, "args.yml")) as f:
            self.h = dict(yaml.safe_load(f))
        self.device = torch.device(device if str(device) != "cuda" else "cuda:0")
        self._net = None

    def net(self):
        from .engine import Context, build_bigvgan
        if self._net is None:
            self._net = build_bigvgan(Context(self.device), self.state, self.h, precision=self.precision)
        return self._net

    def vocode(self, spec):
        """spec [80,T] numpy or [B,80,T] tensor -> squeezed float32 numpy waveform (models.py:406-411)."""
        if isinstance(spec, np.ndarray):
            spec = torch.from_numpy(spec).unsqueeze(0)
        spec = spec.to(dtype=torch.float32)
        return self.net().run(spec).squeeze().cpu().numpy()

    def vocode_batch(self, spec_bct: Tensor, lengths=None, chunk=None, halo: int = 32) -> Tensor:
        """device-resident batched path (addition; the counterpart of HifiGAN.spec2wav_batch): spec [B,80,T] -> wav [B, T*hop], no host
        round trip.  lengths (ConvNet.vocode_lens): one length in mel frames per row - mels of different lengths padded to T share the
        call, row b holds lengths[b] * hop samples of the clip alone followed by zeros (bit for bit when lengths[b] and T agree mod 4:
        harness.plan_vocoder_calls groups clips that way), the mel padding is never read.  chunk: long mels in chunks of `chunk` frames
        with `halo` frames of context on both sides, with or without lengths (harness.plan_chunk_calls shows the grid); None is the
        whole-row call."""
        return self.net().vocode_lens(spec_bct, lengths, chunk=chunk, halo=halo).squeeze(1)

    def __call__(self, wav):
        return self.vocode(wav)


def normalize_loudness(wav, target_loudness):
    """scripts/test_final.py:342-347."""
    rms = np.sqrt(np.mean(wav ** 2))
    loudness = 20 * np.log10(rms)
    gain = target_loudness - loudness
    return wav * 10 ** (gain / 20)
