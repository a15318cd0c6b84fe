"""Helper of the Vocos tests: the mel variant of Vocos (padding="center") restated as torch modules under the checkpoint's own key
names, so that `state_dict()` is a valid checkpoint for `v2a_amd.Vocos`.  It runs in any dtype and ends in `torch.istft`, the library call
Vocos itself makes.  `forward(features)` returns the taps the GPU tests compare: after embed + norm, after every block, after the final
LayerNorm, the head logits, S, and the wave.

Weights are seeded, not the default initialisation: gamma in 0.5 .. 1.5, norm weights 1 + 0.3 randn, and the head rows scaled so that
the log-magnitudes pass log 100 (the clip is hit) and the phases span several turns."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

# (C, dim, hidden, depth, n_fft, hop, T)
CASES = [
    (10, 64, 192, 2, 64, 16, 2),        # the shortest wave
    (10, 64, 192, 2, 64, 16, 3),        # shorter than the 7 taps
    (10, 64, 192, 2, 64, 16, 37),
    (10, 64, 192, 2, 64, 32, 9),        # two frames per sample
    (10, 64, 192, 2, 64, 24, 11),       # hop does not divide n_fft
    (20, 96, 160, 3, 128, 32, 70),      # dims that are not powers of two, M past one 64-row tile
    (100, 512, 1536, 8, 1024, 256, 21),     # the real network
    (100, 512, 1536, 8, 1024, 256, 130),    # M past 128 rows, K in chunks
]
BATCH = [2, 3, 3, 2, 3, 2, 2, 2]


class ConvNeXtBlock(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, 7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, hidden)
        self.pwconv2 = nn.Linear(hidden, dim)
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):                                       # (b, dim, T)
        r = x
        x = self.dwconv(x).transpose(1, 2)
        x = self.pwconv2(F.gelu(self.pwconv1(self.norm(x))))
        return r + (self.gamma * x).transpose(1, 2)


class Backbone(nn.Module):
    def __init__(self, C, dim, hidden, depth):
        super().__init__()
        self.embed = nn.Conv1d(C, dim, 7, padding=3)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.convnext = nn.ModuleList([ConvNeXtBlock(dim, hidden) for _ in range(depth)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=1e-6)


class ISTFT(nn.Module):
    def __init__(self, n_fft):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft, periodic=True))


class Head(nn.Module):
    def __init__(self, dim, n_fft):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)
        self.istft = ISTFT(n_fft)


class VocosRef(nn.Module):
    def __init__(self, C, dim, hidden, depth, n_fft, hop, seed=0):
        super().__init__()
        self.n_fft, self.hop = n_fft, hop
        self.backbone = Backbone(C, dim, hidden, depth)
        self.head = Head(dim, n_fft)
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("gamma"):
                    p.copy_(0.5 + torch.rand(p.shape, generator=g))
                elif "norm" in name and name.endswith("weight"):
                    p.copy_(1 + 0.3 * rn(*p.shape))
                elif name.endswith("bias"):
                    p.copy_(0.1 * rn(*p.shape))
                elif name == "head.out.weight":
                    nb = n_fft // 2 + 1
                    w = rn(*p.shape) / math.sqrt(p.shape[1])
                    w[:nb] *= 2.5                                # log-magnitudes of a few units: some pass log 100 = 4.6
                    w[nb:] *= 8.0                                # phases of tens of radians
                    p.copy_(w)
                else:
                    fan_in = p[0].numel()
                    p.copy_(rn(*p.shape) / math.sqrt(fan_in))

    def forward(self, features):
        """features (b, C, T) -> dict of taps, time-major: embed / block{i} / final (b, T, dim), logits (b, T, n_fft + 2),
        S (b, T, bins, 2), wave (b, (T - 1) hop)."""
        taps = {}
        bb = self.backbone
        x = bb.norm(bb.embed(features).transpose(1, 2)).transpose(1, 2)
        taps["embed"] = x.transpose(1, 2)
        for i, blk in enumerate(bb.convnext):
            x = blk(x)
            taps[f"block{i}"] = x.transpose(1, 2)
        y = bb.final_layer_norm(x.transpose(1, 2))
        taps["final"] = y
        logits = self.head.out(y)
        taps["logits"] = logits
        nb = self.n_fft // 2 + 1
        mag = torch.clip(torch.exp(logits[..., :nb]), max=1e2)
        p = logits[..., nb:]
        S = mag * (torch.cos(p) + 1j * torch.sin(p))            # (b, T, bins)
        taps["S"] = torch.view_as_real(S)
        window = torch.hann_window(self.n_fft, periodic=True, dtype=features.dtype, device=features.device)
        taps["wave"] = torch.istft(S.transpose(1, 2), self.n_fft, self.hop, self.n_fft, window, center=True)
        return taps


def make_features(b, C, T, seed):
    """(b, C, T) fp32 log-mel-like frames: a smooth part along time plus noise."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(b, C, 1, generator=g) + torch.cumsum(0.3 * torch.randn(b, C, T, generator=g), 2)
    return (base + 0.5 * torch.randn(b, C, T, generator=g)).contiguous()


_CACHE = {}


def case_data(i, extra_bias=0.0):
    """Case i -> dict(ref fp32 module, sd, x (b, C, T) fp32, t64 taps in float64, t32 taps of torch's CPU fp32 run); computed once, shared,
    never changed by a test."""
    key = (i, extra_bias)
    if key not in _CACHE:
        C, dim, hidden, depth, n_fft, hop, T = CASES[i]
        ref = VocosRef(C, dim, hidden, depth, n_fft, hop, seed=100 + i).eval()
        if extra_bias:
            with torch.no_grad():
                ref.head.out.bias[:n_fft // 2 + 1] += extra_bias
        x = make_features(BATCH[i], C, T, seed=200 + i)
        with torch.no_grad():
            t32 = {k: v.detach() for k, v in ref(x).items()}
            ref64 = VocosRef(C, dim, hidden, depth, n_fft, hop, seed=100 + i).double().eval()
            ref64.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
            t64 = {k: v.detach() for k, v in ref64(x.double()).items()}
        _CACHE[key] = dict(ref=ref, sd={k: v.clone() for k, v in ref.state_dict().items()}, x=x, t64=t64, t32=t32, hop=hop, n_fft=n_fft)
    return _CACHE[key]


def ratio(got, want64):
    """max |x - x64| / max |x64| per clip -> the largest over the clips."""
    got, want64 = got.double().reshape(got.shape[0], -1), want64.reshape(want64.shape[0], -1)
    return float(((got - want64).abs().amax(1) / want64.abs().amax(1)).max())
