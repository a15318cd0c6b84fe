"""CPU: the host restatements behind the Vocos vocoder (v2a_amd.vocos) against torch in float64 -- the inverse-DFT basis against
torch.fft.irfft, the gather overlap-add against torch.istft, the window envelope -- and the properties of the seeded reference network
(tests/vocos_ref.py) that the GPU tests rely on."""
import math

import numpy as np
import pytest
import torch

import vocos_ref as R


def _hann(n):
    return torch.hann_window(n, periodic=True, dtype=torch.float64)


@pytest.mark.parametrize("n_fft", [4, 64, 128, 1024])
def test_basis_times_spectrum_is_windowed_irfft(n_fft):
    """basis @ (re, im) = irfft(S) * w to 1e-13 relative, for S with non-zero imaginary DC and Nyquist parts (a C2R transform ignores them)."""
    from v2a_amd import istft_basis
    nb = n_fft // 2 + 1
    g = torch.Generator().manual_seed(n_fft)
    S = torch.complex(torch.randn(7, nb, generator=g, dtype=torch.float64), torch.randn(7, nb, generator=g, dtype=torch.float64))
    assert float(S[:, 0].imag.abs().min()) > 0 and float(S[:, -1].imag.abs().min()) > 0
    want = torch.fft.irfft(S, n=n_fft) * _hann(n_fft)
    basis = istft_basis(n_fft)
    assert basis.shape == (n_fft, 2 * nb) and basis.dtype == torch.float64
    got = torch.view_as_real(S).reshape(7, -1) @ basis.T
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((basis[:, 1] == 0).all()) and bool((basis[:, 2 * nb - 1] == 0).all())       # exactly zero, not sin(pi j) in float64
    assert float(basis[:, 3].abs().max()) > 0


def test_basis_refuses_bad_sizes():
    from v2a_amd import istft_basis
    for n in (0, 2, 6, 1022):
        with pytest.raises(ValueError, match="n_fft"):
            istft_basis(n)


@pytest.mark.parametrize("n_fft,hop,T", [(64, 16, 2), (64, 16, 3), (64, 16, 37), (64, 32, 9), (64, 24, 11), (128, 32, 70), (64, 64, 4), (64, 1, 5)])
def test_gather_overlap_add_is_torch_istft(n_fft, hop, T):
    """The gather form of v2a_vocos_overlap_add, restated in numpy in float64, equals torch.istft bit for bit."""
    from v2a_amd.vocos import overlap_add_numpy, window_envelope
    g = torch.Generator().manual_seed(T)
    nb = n_fft // 2 + 1
    S = torch.complex(torch.randn(nb, T, generator=g, dtype=torch.float64), torch.randn(nb, T, generator=g, dtype=torch.float64))
    if hop == n_fft:                                                            # the envelope is zero between the frames: torch refuses
        with pytest.raises(RuntimeError):
            torch.istft(S[None], n_fft, hop, n_fft, _hann(n_fft), center=True)
        return
    want = torch.istft(S[None], n_fft, hop, n_fft, _hann(n_fft), center=True)[0].numpy()
    frames = (torch.fft.irfft(S.T, n=n_fft) * _hann(n_fft)).numpy()
    got = overlap_add_numpy(frames, hop)
    assert got.shape == want.shape == ((T - 1) * hop,)
    assert np.array_equal(got, want)
    # the envelope helper is the divisor torch uses
    env = window_envelope(n_fft, hop, T)
    ola = np.zeros((T - 1) * hop + n_fft)
    for t in range(T):
        ola[t * hop:t * hop + n_fft] += frames[t]
    assert np.allclose(ola[n_fft // 2:n_fft // 2 + (T - 1) * hop] / env, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_reference_network_hits_the_clip_and_turns_the_phases(i):
    """What the GPU parity test asserts about its float64 reference, checked here without a GPU, with the figures torch's CPU fp32 run
    of the same restatement gives (1e-7 .. 1e-5 of the peak)."""
    d = R.case_data(i)
    C, dim, hidden, depth, n_fft, hop, T = R.CASES[i]
    nb = n_fft // 2 + 1
    lg = d["t64"]["logits"]
    clipped = float((lg[..., :nb] > math.log(100.0)).double().mean())
    assert 0.001 <= clipped <= 0.5, clipped
    assert float(lg[..., nb:].abs().max()) > 4 * math.pi
    assert d["t64"]["wave"].shape == (R.BATCH[i], (T - 1) * hop)
    assert set(d["t64"]) == {"embed", "final", "logits", "S", "wave"} | {f"block{k}" for k in range(depth)}
    for name, want in d["t64"].items():
        r = R.ratio(d["t32"][name], want)
        assert 0 < r < 1e-4, (name, r)
    sd = d["sd"]
    assert all(0.5 <= float(v.min()) and float(v.max()) <= 1.5 for k, v in sd.items() if k.endswith("gamma"))


def test_reference_state_dict_is_a_checkpoint():
    from v2a_amd.vocos import expected_state_dict_shapes
    d = R.case_data(5)
    C, dim, hidden, depth, n_fft, hop, T = R.CASES[5]
    want = expected_state_dict_shapes(C, dim, hidden, depth, n_fft)
    assert {k: tuple(v.shape) for k, v in d["sd"].items() if k != "head.istft.window"} == want
    assert tuple(d["sd"]["head.istft.window"].shape) == (n_fft,)
    real = expected_state_dict_shapes()
    assert real["backbone.embed.weight"] == (512, 100, 7) and real["head.out.weight"] == (1026, 512) and "backbone.convnext.7.gamma" in real
    assert "backbone.convnext.8.gamma" not in real
