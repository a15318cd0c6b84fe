"""FLAN-T5 prompt encoder on the HIP kernels of include/v2a_cfm.h: the `encode_text` of the reference (x3:1648-1657), which
runs transformers `T5EncoderModel` loaded from ./ckpts/flan-t5-large (x3:1412-1413).

Arithmetic is fp32 end to end (exact-fp32 MFMA GEMMs, fp32 norms, softmax and attention); at the sizes of a prompt the encoder
is bound by its fp32 weight stream (1.23 GB for flan-t5-large), which split-bf16 planes would not shrink.  The relative-position
bucket table is built on the host with the same torch expression as transformers' `_relative_position_bucket` (its float32
log is truncated, a device logf could land on the other side of a boundary) and gathered into a per-length bias on the host.
"""
from __future__ import annotations

import math
import re

import torch

from . import _lib as L
from .weights import read_hf_dir, strip_keys

MAX_LEN = 512


def relative_position_bucket_table(n: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """Bucket of every relative position j - i = -(n-1) .. n-1 (int64, length 2n-1), bidirectional: the expression of
    transformers T5Attention._relative_position_bucket, on the 1-D vector of distinct offsets."""
    rel = torch.arange(-(n - 1), n, dtype=torch.long)
    nb = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    max_exact = nb // 2
    is_small = rel < max_exact
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rel, large)


_PREFIXES = ("text_encoder2.",)


def infer_config(sd: dict[str, torch.Tensor]) -> dict:
    """Shapes -> config: layers from the block keys, H from the relative bias, d_kv from q, d_ff from wi_0."""
    emb = sd.get("encoder.embed_tokens.weight", sd.get("shared.weight"))
    if emb is None:
        raise KeyError("T5Encoder: neither shared.weight nor encoder.embed_tokens.weight is in the state dict")
    layers = 1 + max(int(m.group(1)) for m in (re.match(r"encoder\.block\.(\d+)\.", k) for k in sd) if m)
    rb = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    H = rb.shape[1]
    inner = sd["encoder.block.0.layer.0.SelfAttention.q.weight"].shape[0]
    return dict(vocab_size=emb.shape[0], d_model=emb.shape[1], num_heads=H, d_kv=inner // H, num_layers=layers,
                d_ff=sd["encoder.block.0.layer.1.DenseReluDense.wi_0.weight"].shape[0], relative_attention_num_buckets=rb.shape[0],
                relative_attention_max_distance=128, layer_norm_epsilon=1e-6)


def pack_geglu(wi_0: torch.Tensor, wi_1: torch.Tensor) -> torch.Tensor:
    """[16 value | 16 gate] row packing of V2A_EPI_GEGLU_TANH: value = wi_1, gate = wi_0, per group of 16 outputs."""
    f, d = wi_0.shape
    return torch.stack([wi_1.reshape(f // 16, 16, d), wi_0.reshape(f // 16, 16, d)], 1).reshape(2 * f, d)


class T5Encoder:
    """transformers T5EncoderModel (gated-gelu, pre-norm, no biases) on the HIP kernels; fp32.

    `T5Encoder(state_dict, device, tokenizer=None, config=None)`: plain T5EncoderModel keys (`shared.weight` and / or
    `encoder.embed_tokens.weight`) or a reference checkpoint's `text_encoder2.*`; the config is inferred from the shapes unless
    given (a dict of T5Config fields)."""

    def __init__(self, state_dict, device, tokenizer=None, config: dict | None = None):
        sd = strip_keys(state_dict, _PREFIXES)
        cfg = infer_config(sd)
        if config is not None:
            cfg.update({k: v for k, v in dict(config).items() if k in cfg})
        if cfg["d_kv"] != 64:
            raise ValueError(f"T5Encoder: d_kv = {cfg['d_kv']}, the attention kernel is built for 64")
        d, H, dff = cfg["d_model"], cfg["num_heads"], cfg["d_ff"]
        if d % 32 or dff % 32:
            raise ValueError(f"T5Encoder: d_model ({d}) and d_ff ({dff}) must be multiples of 32")
        self.cfg, self.tokenizer = cfg, tokenizer
        self.device = torch.device(device)
        self.inner = H * 64
        dev = lambda t: t.detach().to(self.device, torch.float32).contiguous()
        g = lambda k: sd[k].detach().to("cpu", torch.float32)
        emb = sd.get("encoder.embed_tokens.weight", sd.get("shared.weight"))
        self.embed = dev(emb)
        self.rel_bias = g("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")     # (num_buckets, H), host
        self.layers = []
        for i in range(cfg["num_layers"]):
            P = f"encoder.block.{i}.layer."
            self.layers.append(dict(
                ln1=dev(g(P + "0.layer_norm.weight")),
                qkv=dev(torch.cat([g(P + "0.SelfAttention.q.weight"), g(P + "0.SelfAttention.k.weight"),
                                   g(P + "0.SelfAttention.v.weight")], 0)),
                o=dev(g(P + "0.SelfAttention.o.weight")),
                ln2=dev(g(P + "1.layer_norm.weight")),
                wi=dev(pack_geglu(g(P + "1.DenseReluDense.wi_0.weight"), g(P + "1.DenseReluDense.wi_1.weight"))),
                wo=dev(g(P + "1.DenseReluDense.wo.weight"))))
        self.final_ln = dev(g("encoder.final_layer_norm.weight"))
        self._bias_cache: dict[int, torch.Tensor] = {}
        self._bufs: dict[tuple, dict] = {}
        L.lib()

    @classmethod
    def from_pretrained(cls, path: str, device):
        """A local HF directory (the reference's ./ckpts/flan-t5-large): config.json, weights, tokenizer."""
        from transformers import AutoTokenizer
        hc, sd = read_hf_dir(path)
        if hc.get("feed_forward_proj", "gated-gelu") != "gated-gelu":
            raise NotImplementedError(f"T5Encoder: feed_forward_proj {hc.get('feed_forward_proj')!r} (gated-gelu only)")
        config = {k: hc[k] for k in ("relative_attention_max_distance", "layer_norm_epsilon") if k in hc}
        return cls(sd, device, AutoTokenizer.from_pretrained(path), config)

    # ---- host-side pieces ---------------------------------------------------------------------------
    def position_bias(self, n: int) -> torch.Tensor:
        """(H, 2n-1) fp32 on the device: rel_bias[bucket(j - i)][h] at offset j - i + n - 1."""
        b = self._bias_cache.get(n)
        if b is None:
            tab = relative_position_bucket_table(n, self.cfg["relative_attention_num_buckets"], self.cfg["relative_attention_max_distance"])
            b = self.rel_bias[tab].t().contiguous().to(self.device)
            self._bias_cache[n] = b
        return b

    def _buffers(self, B: int, N: int) -> dict:
        key = (B, N)
        bf = self._bufs.get(key)
        if bf is None:
            M, d, e = B * N, self.cfg["d_model"], lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
            bf = dict(h=e(M, d), x=e(M, d), qkv=e(M, 3 * self.inner), ao=e(M, self.inner), ff=e(M, self.cfg["d_ff"]))
            self._bufs = {key: bf}            # one live shape: prompts of a call share it
        return bf

    # ---- the encoder ------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_ids(self, input_ids, attention_mask=None, *, taps: dict | None = None):
        """input_ids (B, N) int, attention_mask (B, N) 0/1 or bool (None = all valid) -> (hidden (B, N, d) fp32 on the device,
        mask (B, N) bool on the device).  `taps`: a dict whose keys are layer numbers 1..L; each receives a device copy of the
        residual stream after that block (before the final norm)."""
        ids = torch.as_tensor(input_ids)
        if ids.ndim != 2:
            raise ValueError(f"input_ids must be (B, N), got {tuple(ids.shape)}")
        B, N = ids.shape
        if N < 1 or N > MAX_LEN:
            raise ValueError(f"T5Encoder: N = {N} tokens, 1..{MAX_LEN} supported")
        mask = torch.ones(B, N, dtype=torch.int32) if attention_mask is None else torch.as_tensor(attention_mask).to("cpu").to(torch.int32)
        if tuple(mask.shape) != (B, N):
            raise ValueError(f"attention_mask {tuple(mask.shape)} does not match input_ids {(B, N)}")
        ids_h = ids.to("cpu", torch.int64)
        V = self.cfg["vocab_size"]
        if bool((ids_h < 0).any()) or bool((ids_h >= V).any()):
            raise ValueError(f"T5Encoder: token id out of range [0, {V})")
        if not bool((mask != 0).any(1).all()):
            raise ValueError("T5Encoder: a batch row has no valid key (attention_mask all zero)")
        mask = (mask != 0).to(torch.int32)
        c, d, H, dff, inner, eps = self.cfg, self.cfg["d_model"], self.cfg["num_heads"], self.cfg["d_ff"], self.inner, self.cfg["layer_norm_epsilon"]
        M = B * N
        ids_d = ids_h.to(torch.int32).to(self.device)
        mask_d = mask.to(self.device)
        bias = self.position_bias(N)
        bf = self._buffers(B, N)
        h, x, qkv, ao, ff = bf["h"], bf["x"], bf["qkv"], bf["ao"], bf["ff"]
        L.t5_rmsnorm(self.embed, x, self.layers[0]["ln1"], rows=M, d=d, eps=eps, ids=ids_d, vocab=V, resid=h)
        for li, Lw in enumerate(self.layers):
            if li > 0:
                L.t5_rmsnorm(h, x, Lw["ln1"], rows=M, d=d, eps=eps)
            L.gemm_skinny(x, Lw["qkv"], qkv, M=M, N=3 * inner, K=d)
            L.t5_attention(qkv, ao, bias, mask_d, B=B, H=H, N=N, inner=inner)
            L.gemm_skinny(ao, Lw["o"], h, M=M, N=d, K=inner, epilogue=L.EPI_RESID, resid=h)
            L.t5_rmsnorm(h, x, Lw["ln2"], rows=M, d=d, eps=eps)
            L.gemm_skinny(x, Lw["wi"], ff, M=M, N=2 * dff, K=d, epilogue=L.EPI_GEGLU_TANH)
            L.gemm_skinny(ff, Lw["wo"], h, M=M, N=d, K=dff, epilogue=L.EPI_RESID, resid=h)
            if taps is not None and li + 1 in taps:
                taps[li + 1] = h.view(B, N, d).clone()
        out = torch.empty(M, d, dtype=torch.float32, device=self.device)
        L.t5_rmsnorm(h, out, self.final_ln, rows=M, d=d, eps=eps)
        return out.view(B, N, d), mask_d.to(torch.bool)

    def tokenize(self, prompts):
        """x3:1650: padding to the longest prompt, truncation at model_max_length."""
        if self.tokenizer is None:
            raise RuntimeError("T5Encoder: no tokenizer (construct with tokenizer= or use from_pretrained)")
        tok = self.tokenizer
        b = tok(list(prompts), max_length=min(getattr(tok, "model_max_length", MAX_LEN), MAX_LEN), padding=True, truncation=True,
                return_tensors="pt")
        return b["input_ids"], b["attention_mask"]

    def __call__(self, prompts):
        """encode_text x3:1648-1657: prompts -> (hidden (B, N, d) fp32, mask (B, N) bool), both on the device."""
        if isinstance(prompts, str):
            prompts = [prompts]
        ids, am = self.tokenize(prompts)
        return self.encode_ids(ids, am)
